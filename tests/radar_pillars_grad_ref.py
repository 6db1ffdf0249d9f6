"""The radar pillar branch in TRAINING mode, restated for the tests of its HIP route (racformer_amd/radar_pillars.py,
``RadarPillarEncoder.fused_grad``): ``radar_pillars_ref.Stages`` (torch.nn modules, its own decoration and scatter; nothing shared
with the module under test) with every BatchNorm on batch statistics, in float64 or float32 on the CPU, under autograd.

The two kinds of decisions of the branch can be imposed from outside, so that a route whose float32 value fell on the other side of a
tie is compared on the function it actually differentiated:
  * the PFN layer's winning slot per (pillar, channel) (-1: a padded slot) and whether the winner is above the ReLU's zero,
  * the ReLU mask of every ConvModule's output.
The criterion is tests/test_resnet_grad_gpu.py's: err < max(4 x E_ref, 1e-5 x max|want|) per tensor, E_ref the float32 run of the same
computation with the same imposed decisions against the float64 run."""
import torch

import radar_pillars_ref as R

PFN_MOMENTUM = 0.01                 # the reference's norm_cfg for the PFN layer (Stages builds it with torch's default)
PARAMS = ["radar_voxel_encoder.pfn_layers.0.linear.weight", "radar_voxel_encoder.pfn_layers.0.norm.weight",
          "radar_voxel_encoder.pfn_layers.0.norm.bias"] + [f"radar_bev_conv.{i}.{n}" for i in range(3)
                                                           for n in ("conv.weight", "bn.weight", "bn.bias")]
BUFFERS = [f"{p}.{n}" for p in ["radar_voxel_encoder.pfn_layers.0.norm"] + [f"radar_bev_conv.{i}.bn" for i in range(3)]
           for n in ("running_mean", "running_var", "num_batches_tracked")]


class TrainStages:
    """``Stages`` with the BatchNorms in training mode; parameters require gradients."""

    def __init__(self, sd, dtype, cfg):
        self.st = st = R.Stages(sd, dtype, **cfg)
        self.dtype = dtype
        st.norm.momentum = PFN_MOMENTUM
        st.norm.train()
        for _, bn in st.convs:
            bn.train()
        self.modules = {"radar_voxel_encoder.pfn_layers.0.linear": st.linear, "radar_voxel_encoder.pfn_layers.0.norm": st.norm}
        for i, (conv, bn) in enumerate(st.convs):
            self.modules[f"radar_bev_conv.{i}.conv"], self.modules[f"radar_bev_conv.{i}.bn"] = conv, bn

    def tensor(self, name):
        mod, attr = name.rsplit(".", 1)
        return getattr(self.modules[mod], attr)

    def pfn(self, voxels, coors, num, slots=None, pos=None):
        """-> (feats [M, 64], own slots [M, 64] (first maximum, -1 = padded), the winner's pre-activation [M, 64], all
        pre-activations [M, P, 64]).  ``slots`` / ``pos`` impose the winner and its ReLU decision."""
        st = self.st
        M, P = voxels.shape[:2]
        if M == 0:
            z = torch.zeros(0, 64, dtype=self.dtype)
            return z, torch.zeros(0, 64, dtype=torch.long), z, torch.zeros(0, P, 64, dtype=self.dtype)
        f = st.decorate(voxels, coors, num)
        pre = st.norm(st.linear(f).transpose(1, 2)).transpose(1, 2)                       # [M, P, 64]
        own = first_max_slots(torch.relu(pre.detach()), num)
        use = own if slots is None else slots
        # a padded winner: any padded row of the pillar carries its value (they are all the same row of zeros)
        idx = torch.where(use < 0, num.long().view(-1, 1).expand(-1, 64).clamp(max=P - 1), use.long())
        win = pre.gather(1, idx.unsqueeze(1)).squeeze(1)
        feats = torch.relu(win) if pos is None else win * pos.to(self.dtype)
        return feats, own, win, pre

    def scatter(self, feats, coors, batch):
        st = self.st
        canvas = torch.zeros(batch, 64, st.grid[1], st.grid[0], dtype=self.dtype)
        if feats.shape[0] == 0:
            return canvas
        return _scatter(canvas, coors.long(), feats)

    def conv_layer(self, i, x, mask=None):
        """-> (output, pre-activation); ``mask`` imposes the ReLU decision"""
        conv, bn = self.st.convs[i]
        pre = bn(conv(x.to(self.dtype)))
        return (torch.relu(pre) if mask is None else pre * mask.to(self.dtype)), pre


def _scatter(canvas, c, feats):
    canvas = canvas.clone()
    canvas[c[:, 0], :, c[:, 2], c[:, 3]] = feats
    return canvas


def first_max_slots(y, num):
    """y [M, P, 64] post-ReLU (padded rows included) -> the first slot holding the maximum, -1 where that slot is padded"""
    P = y.shape[1]
    best = y.max(dim=1, keepdim=True)[0]
    first = torch.where(y == best, torch.arange(P).view(1, P, 1), torch.full((1, 1, 1), P)).min(dim=1)[0]
    return torch.where(first >= num.long().view(-1, 1), torch.full_like(first, -1), first)


def branch(ts, voxels, coors, num, batch, decisions=None):
    """The whole branch -> (output [B, 256, H, W], dict of the run's own decisions and pre-activations).  ``decisions``:
    dict(slots, pos, masks = [3 masks]) to impose, or None."""
    d = decisions or {}
    feats, own, win, pre = ts.pfn(voxels, coors, num, d.get("slots"), d.get("pos"))
    x = ts.scatter(feats, coors, batch)
    info = dict(slots=own, win=win, pre=pre, canvas=x, layer_pre=[], layer_out=[])
    for i in range(3):
        x, p = ts.conv_layer(i, x, d["masks"][i] if "masks" in d else None)
        info["layer_pre"].append(p)
        info["layer_out"].append(x)
    return x, info


def grads_and_buffers(sd, cfg, dtype, voxels, coors, num, batch, gout, decisions=None, names=PARAMS):
    """One training step's forward + backward -> (output, {parameter: grad}, {buffer: value after the step}, info)."""
    ts = TrainStages(sd, dtype, cfg)
    for n in PARAMS:
        ts.tensor(n).requires_grad_(n in names)
    out, info = branch(ts, voxels, coors, num, batch, decisions)
    out.backward(gout.to(dtype))
    grads = {n: ts.tensor(n).grad for n in names}
    return out.detach(), grads, {n: ts.tensor(n).detach().clone() for n in BUFFERS}, info


def bound(want, ref32):
    """the criterion's allowance for one tensor"""
    want, ref32 = want.detach().double(), ref32.detach()
    e_ref =float((ref32.double() - want).abs().max()) if want.numel() else 0.0
    big = float(want.abs().max()) if want.numel() else 0.0
    return max(4.0 * e_ref, 1e-5 * big), e_ref, big


def hold(what, got, want, ref32):
    allow, e_ref, big = bound(want, ref32)
    got = got.detach().double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} against {tuple(want.shape)}"
    err = float((got - want.double()).abs().max()) if want.numel() else 0.0
    print(f"\n{what}: err {err:.3e}  E_ref {e_ref:.3e}  max|want| {big:.3e}")
    if big == 0.0 and e_ref == 0.0:
        assert err == 0.0, f"{what}: {err:.3e} where the reference is exactly zero"
    else:
        assert err < allow, f"{what}: {err:.3e} against E_ref {e_ref:.3e}, max|want| {big:.3e}"
    return err
