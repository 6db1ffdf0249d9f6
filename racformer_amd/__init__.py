"""racformer_amd — MI355X-native (gfx950) implementation of RaCFormer's query-decoder hot path.

Only what the path needs lives here: ``csrc/`` (hand-written HIP kernels behind a C-ABI,
``include/racformer_hip.h``) and host-side mirrors of the reference's operator/plugin surface
(``msmv_sampling``, ``MultiScaleDeformableAttnFunction_fp32``, ``sampling_4d``,
``RaCFormerTransformer``, ``RaCFormer_head``, ``LSSViewTransformer_racformer``).  The compute path has no CPU fallback: ops raise
if the HIP library is missing or a tensor is not on the GPU.
"""
__version__ = "0.1.0"

from .lss_view import (LSSViewFunction, LSSViewTransformer_racformer, lss_cells, lss_rank_tables,  # noqa: E402,F401
                       lss_view_backward, lss_view_forward, lss_view_transform)
from .lss_depth import (LSSViewTransformerBEVDepth_racformer, depth_loss, pool_bins, radar_prior)  # noqa: E402,F401
from .depth_net import DepthNet  # noqa: E402,F401
from .necks import FPN, CustomFPN  # noqa: E402,F401
from .resnet import ResNet  # noqa: E402,F401
from .detector import RaCFormer  # noqa: E402,F401
from .optim import CosineAnnealingLr, FusedAdamW, build_optimizer, parse_losses, train_step  # noqa: E402,F401
