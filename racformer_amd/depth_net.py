"""``DepthNet`` of ``LSSViewTransformerBEVDepth_racformer`` (models/necks/view_transformer_racformer.py:329-567 of the reference):
image features of the LSS neck plus the radar priors -> depth logits and context features, ``[B*N, D + context, h, w]`` -- the
tensor whose two views ``lss_view`` takes.  The reference's constructor arguments, ``forward`` signature and state-dict keys
(``reduce_conv.{0,1}``, ``bn``, ``{depth,context}_mlp.fc{1,2}``, ``{depth,context}_se.conv_{reduce,expand}``, ``dep_proj``,
``depth_conv.{0,1,2}.{conv1,bn1,conv2,bn2}``, ``depth_conv.3.aspp{1..4}.{atrous_conv,bn}``, ``depth_conv.3.global_avg_pool.{1,2}``,
``depth_conv.3.{conv1,bn1}``, ``depth_conv.4``, ``context_conv``), so a reference checkpoint loads with ``strict=True``.
``BasicBlock`` restates mmdet 2.28.2's (conv3x3 without bias, BN, ReLU, conv3x3, BN, + identity, ReLU) and ``build_norm``
mmcv 1.6.0's ``build_norm_layer`` for the types the reference's configs name.  DCN (``use_dcn=True``) is not implemented: the f8
configuration sets ``use_dcn=False`` and no configuration of the reference enables it.

Two routes:
  torch   plain ``nn`` modules on any device and dtype, training mode and autograd included; taken for CPU tensors, float64,
          ``depth_only=True``, the LayerNorm(9) variant of ``norm_cfg`` GN / SyncBN, ``mid_channels != 256``, ``fused=False``,
          ``train()`` and whenever a gradient is required.  It is the oracle of the other route.
  HIP     device float32 tensors, ``eval()``, no gradient, ``in_channels == mid_channels == 256``, ``norm_cfg`` BN: the kernels of
          ``csrc/depth_net.hip`` (``rac_conv_small_*``, ``rac_depthnet_*``).  Every BatchNorm is folded into its neighbour in
          float64 once per weight version; no torch or library convolution / GEMM runs, nothing is read back, the launches are
          sized by shapes: capturable into a graph, and two runs give the same bits.

On the HIP route the activations between layers are channel-last rows.  The SE gates scale the input channels of
``context_conv`` and ``dep_proj`` while the kernel stages them; the image-pool branch of ASPP is a per-image bias of its
``conv1``; ASPP's four branches write straight into the rows ``conv1`` reads.  ``dep_proj``'s 129 prior channels are two table
lookups (``forward_fused``: one column of its weight per depth bin, one precomputed row per RCS class); the drop-in ``forward``
takes the two dense tensors and runs them through the same kernel as 160 more (zero-padded) input channels.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .radar_pillars import _param_sig, fold_bn

HIP_CHANNELS = 256
trace = None   # tools/depth_net_bench.py sets a list: every launch appends (entry point, label, workgroups)


def _note(entry, label, workgroups):
    if trace is not None:
        trace.append((entry, label, workgroups))

DCN_MESSAGE = ("DepthNet: use_dcn=True (mmcv's deformable convolution) is not implemented; the f8 configuration "
               "(configs/racformer_r50_nuimg_704x256_f8.py) sets depthnet_cfg=dict(use_dcn=False) -- pass use_dcn=False")


def build_norm(norm_cfg, num_features):
    """mmcv 1.6.0 ``build_norm_layer(cfg, num_features)[1]`` for BN / BN2d / SyncBN / GN: eps defaults to 1e-5, the other keys of
    the config go to the layer; ``requires_grad`` (default True) is applied to its parameters."""
    cfg = dict(norm_cfg)
    kind = cfg.pop("type")
    requires_grad = cfg.pop("requires_grad", True)
    cfg.setdefault("eps", 1e-5)
    if kind in ("BN", "BN2d"):
        layer = nn.BatchNorm2d(num_features, **cfg)
    elif kind == "SyncBN":
        layer = nn.SyncBatchNorm(num_features, **cfg)
    elif kind == "GN":
        layer = nn.GroupNorm(num_channels=num_features, **cfg)
    else:
        raise KeyError(f"DepthNet: unsupported norm_cfg type {kind!r} (BN, BN2d, SyncBN or GN)")
    for p in layer.parameters():
        p.requires_grad = requires_grad
    return layer


class BasicBlock(nn.Module):
    """mmdet 2.28.2 ``BasicBlock(inplanes, planes)`` at stride 1 without downsample."""

    def __init__(self, inplanes, planes, norm_cfg=dict(type='BN')):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=1, padding=1, dilation=1, bias=False)
        self.bn1 = build_norm(norm_cfg, planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = build_norm(norm_cfg, planes)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + x)


class _ASPPModule(nn.Module):
    def __init__(self, inplanes, planes, kernel_size, padding, dilation, norm_cfg=dict(type='BN')):
        super().__init__()
        self.atrous_conv = nn.Conv2d(inplanes, planes, kernel_size=kernel_size, stride=1, padding=padding, dilation=dilation,
                                     bias=False)
        self.bn = build_norm(norm_cfg, planes)
        self.relu = nn.ReLU()
        _init_weight(self)

    def forward(self, x):
        return self.relu(self.bn(self.atrous_conv(x)))


def _init_weight(module):
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            torch.nn.init.kaiming_normal_(m.weight)
        elif isinstance(m, nn.BatchNorm2d):
            m.weight.data.fill_(1)
            m.bias.data.zero_()


class ASPP(nn.Module):
    DILATIONS = (1, 6, 12, 18)

    def __init__(self, inplanes, mid_channels=256, norm_cfg=dict(type='BN')):
        super().__init__()
        d = self.DILATIONS
        self.aspp1 = _ASPPModule(inplanes, mid_channels, 1, padding=0, dilation=d[0], norm_cfg=norm_cfg)
        self.aspp2 = _ASPPModule(inplanes, mid_channels, 3, padding=d[1], dilation=d[1], norm_cfg=norm_cfg)
        self.aspp3 = _ASPPModule(inplanes, mid_channels, 3, padding=d[2], dilation=d[2], norm_cfg=norm_cfg)
        self.aspp4 = _ASPPModule(inplanes, mid_channels, 3, padding=d[3], dilation=d[3], norm_cfg=norm_cfg)
        self.global_avg_pool = nn.Sequential(nn.AdaptiveAvgPool2d((1, 1)), nn.Conv2d(inplanes, mid_channels, 1, stride=1, bias=False),
                                             build_norm(norm_cfg, mid_channels), nn.ReLU())
        self.conv1 = nn.Conv2d(int(mid_channels * 5), mid_channels, 1, bias=False)
        self.bn1 = build_norm(norm_cfg, mid_channels)
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(0.5)
        _init_weight(self)

    def forward(self, x):
        x1, x2, x3, x4 = self.aspp1(x), self.aspp2(x), self.aspp3(x), self.aspp4(x)
        x5 = F.interpolate(self.global_avg_pool(x), size=x4.size()[2:], mode='bilinear', align_corners=True)
        x = torch.cat((x1, x2, x3, x4, x5), dim=1)
        return self.dropout(self.relu(self.bn1(self.conv1(x))))


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.ReLU, drop=0.0):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.drop1 = nn.Dropout(drop)
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop2 = nn.Dropout(drop)

    def forward(self, x):
        return self.drop2(self.fc2(self.drop1(self.act(self.fc1(x)))))


class SELayer(nn.Module):
    def __init__(self, channels, act_layer=nn.ReLU, gate_layer=nn.Sigmoid):
        super().__init__()
        self.conv_reduce = nn.Conv2d(channels, channels, 1, bias=True)
        self.act1 = act_layer()
        self.conv_expand = nn.Conv2d(channels, channels, 1, bias=True)
        self.gate = gate_layer()

    def forward(self, x, x_se):
        return x * self.gate(self.conv_expand(self.act1(self.conv_reduce(x_se))))


# ---------------------------------------------------------------------------------------------------------------- packing
def _fold(conv, bn):
    """(conv with or without bias, BatchNorm in eval) -> (weight * g, (bias - mean) * g + beta), folded in float64"""
    w, shift = fold_bn(conv.weight, bn)
    if conv.bias is not None:
        g = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        shift = (shift.double() + conv.bias.detach().double() * g).float()
    return w, shift


def pack_conv_small(weight, cout_multiple=64):
    """[Cout, Cin, k, k] -> the operand of ``rac_conv_small_fwd``: float32 [k*k, Cin, ld_w], ld_w = Cout rounded up, zero-padded"""
    co, ci, kh, kw = weight.shape
    ld = -(-co // cout_multiple) * cout_multiple
    out = weight.new_zeros(kh * kw, ci, ld, dtype=torch.float32)
    out[:, :, :co] = weight.detach().float().permute(2, 3, 1, 0).reshape(kh * kw, ci, co)
    return out.contiguous()


def conv_small(x, w, cout, H, W, ksize=1, dilation=1, cin=None, bias=None, img_bias=None, gate=None, residual=None, bins=None,
               bins_table=None, cls=None, cls_table=None, relu=False, out=None, channel_first=False, c_off=0):
    """One ``rac_conv_small_fwd`` launch.  x: channel-last rows [BN, H*W, ld_in]; w: ``pack_conv_small``'s operand; out: the
    destination ([BN, H*W, ld_out] rows, or [BN, C_total, H, W] with ``channel_first``), allocated at ``cout`` channels if None."""
    BN, hw, ld_in = x.shape
    d = _lib.ConvSmall()
    if out is None:
        out = torch.empty((BN, cout, H, W) if channel_first else (BN, hw, cout), dtype=torch.float32, device=x.device)
    p = lambda t: t.data_ptr() if t is not None else None        # noqa: E731
    d.in_, d.w, d.bias, d.img_bias, d.gate, d.residual = p(x), p(w), p(bias), p(img_bias), p(gate), p(residual)
    d.bins, d.bins_table, d.cls, d.cls_table, d.out = p(bins), p(bins_table), p(cls), p(cls_table), p(out)
    d.BN, d.H, d.W, d.Cin, d.Cout, d.ksize, d.dilation = BN, H, W, (w.shape[1] if cin is None else cin), cout, ksize, dilation
    d.ld_in, d.ld_w = ld_in, w.shape[2]
    d.gate_channels = gate.shape[-1] if gate is not None else 0
    d.ld_res = residual.shape[-1] if residual is not None else 0
    d.n_bins = bins_table.shape[0] if bins_table is not None else 0
    d.n_cls = cls_table.shape[0] - 1 if cls_table is not None else 0
    d.relu, d.out_layout = int(relu), (_lib.CS_CHANNEL_FIRST if channel_first else _lib.CS_CHANNEL_LAST)
    d.ld_out, d.c_off = (out.shape[1] if channel_first else out.shape[2]), c_off
    _lib.check(_lib.lib().rac_conv_small_fwd(_lib.ctypes.byref(d), _lib.stream_ptr()), "rac_conv_small_fwd")
    _note("rac_conv_small_fwd", f"{ksize}x{ksize} d{dilation} {d.Cin}->{cout}", BN * -(-hw // 64) * -(-cout // 64))
    return out


def pack_rows(src, dst, c_off=0, c_pad=0):
    """``rac_conv_small_pack_fwd``: channel-first src [BN, C, h, w] into channels c_off.. of the rows dst [BN, h*w, ld], zeros in
    the c_pad channels behind them."""
    BN, C, h, w = src.shape
    rc = _lib.lib().rac_conv_small_pack_fwd(_lib.ptr(src), _lib.ptr(dst), BN, C, h * w, dst.shape[2], c_off, c_pad, _lib.stream_ptr())
    _lib.check(rc, "rac_conv_small_pack_fwd")
    _note("rac_conv_small_pack_fwd", f"{C}+{c_pad} channels", BN * -(-h * w // 32) * -(-(C + c_pad) // 32))
    return dst


def _t(w):
    """Linear / 1x1 weight [out, in(, 1, 1)] -> [in, out] float64"""
    return w.detach().double().reshape(w.shape[0], -1).t()


class DepthNet(nn.Module):
    def __init__(self, in_channels, mid_channels, context_channels, depth_channels, use_dcn=True, use_aspp=True, depth_only=False,
                 norm_cfg=dict(type='BN'), fused=True):
        super().__init__()
        if use_dcn:
            raise NotImplementedError(DCN_MESSAGE)
        self.depth_only = depth_only
        self.in_channels, self.mid_channels = in_channels, mid_channels
        self.context_channels, self.depth_channels = context_channels, depth_channels
        self.use_aspp, self.norm_type, self.fused = use_aspp, norm_cfg['type'], fused
        self.reduce_conv = nn.Sequential(nn.Conv2d(in_channels, mid_channels, kernel_size=3, stride=1, padding=1),
                                         build_norm(norm_cfg, mid_channels), nn.ReLU(inplace=True))
        self.context_conv = nn.Conv2d(mid_channels, context_channels, kernel_size=1, stride=1, padding=0)
        self.bn = nn.LayerNorm(9) if norm_cfg['type'] in ('GN', 'SyncBN') else nn.BatchNorm1d(9)
        self.depth_mlp = Mlp(9, mid_channels, mid_channels)
        self.depth_se = SELayer(mid_channels)
        self.dep_proj = nn.Conv2d(mid_channels + depth_channels + 1 + 32, mid_channels, kernel_size=1, stride=1, padding=0)
        self.context_mlp = Mlp(9, mid_channels, mid_channels)
        self.context_se = SELayer(mid_channels)
        layers = [BasicBlock(mid_channels, mid_channels, norm_cfg=norm_cfg) for _ in range(3)]
        if use_aspp:
            layers.append(ASPP(mid_channels, mid_channels, norm_cfg=norm_cfg))
        layers.append(nn.Conv2d(mid_channels, depth_channels, kernel_size=1, stride=1, padding=0))
        self.depth_conv = nn.Sequential(*layers)
        if depth_only:
            del self.context_mlp
            del self.context_se
            del self.context_conv
        self._packed = None
        self._tables = None

    # ------------------------------------------------------------------------------------------------------------ torch route
    def forward_torch(self, x, radar_feats, rcs_embedding, mlp_input):
        mlp_input = self.bn(mlp_input.reshape(-1, mlp_input.shape[-1]))
        x = self.reduce_conv(x)
        depth_se = self.depth_mlp(mlp_input)[..., None, None]
        depth = self.depth_se(x, depth_se)
        if self.depth_only:
            return self.depth_conv(depth)
        context_se = self.context_mlp(mlp_input)[..., None, None]
        context = self.context_conv(self.context_se(x, context_se))
        depth = self.dep_proj(torch.cat((depth, radar_feats, rcs_embedding), dim=1))
        return torch.cat([self.depth_conv(depth), context], dim=1)

    # ------------------------------------------------------------------------------------------------------------ HIP route
    def hip_route(self, x, mlp_input, *others):
        """True if this call runs on the kernels (the conditions of the module docstring)."""
        if not self.fused or self.training or self.depth_only or self.norm_type not in ('BN', 'BN2d'):
            return False
        if self.in_channels != HIP_CHANNELS or self.mid_channels != HIP_CHANNELS:
            return False
        tensors = [x, mlp_input] + [t for t in others if t is not None]
        if not all(t.is_cuda for t in tensors) or x.dtype != torch.float32 or mlp_input.dtype != torch.float32:
            return False
        if any(t.dtype not in (torch.float32, torch.int32) for t in tensors):
            return False
        if any(p.dtype != torch.float32 or not p.is_cuda for p in self.parameters()):
            return False
        if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or any(p.requires_grad for p in self.parameters())):
            return False
        return True

    def packed(self):
        """The folded and packed operands, rebuilt when a parameter or buffer changes (``radar_pillars.py``'s signature rule)."""
        sig = _param_sig(self)
        if self._packed is not None and self._packed[0] == sig:
            return self._packed[1]
        C, D = self.mid_channels, self.depth_channels
        f32 = lambda t: t.detach().to(torch.float32, copy=True).contiguous()       # noqa: E731  (a copy: never an alias of a parameter)
        pk = {}
        w, b = _fold(self.reduce_conv[0], self.reduce_conv[1])
        pk["reduce"] = (pack_conv_small(w), b)
        # BatchNorm1d(9) in front of both Mlps: fc1(bn(x)) = (W1 g) x + (W1 s + b1)
        g9 = self.bn.weight.detach().double() / torch.sqrt(self.bn.running_var.detach().double() + self.bn.eps)
        s9 = self.bn.bias.detach().double() - self.bn.running_mean.detach().double() * g9
        blocks = []
        for mlp, se in ((self.context_mlp, self.context_se), (self.depth_mlp, self.depth_se)):
            w1 = mlp.fc1.weight.detach().double()
            parts = [(w1 * g9).t(), w1 @ s9 + mlp.fc1.bias.detach().double(), _t(mlp.fc2.weight), mlp.fc2.bias.detach().double(),
                     _t(se.conv_reduce.weight), se.conv_reduce.bias.detach().double(), _t(se.conv_expand.weight),
                     se.conv_expand.bias.detach().double()]
            blocks.append(torch.cat([p.contiguous().reshape(-1) for p in parts]))
        pk["gates"] = f32(torch.stack(blocks))
        pk["context"] = (pack_conv_small(self.context_conv.weight), f32(self.context_conv.bias.detach()))
        wd = self.dep_proj.weight.detach()
        pk["dep_x"] = pack_conv_small(wd[:, :C])
        cin_dense = -(-wd.shape[1] // 32) * 32
        dense = wd.new_zeros(wd.shape[0], cin_dense, 1, 1)
        dense[:, :wd.shape[1]] = wd
        pk["dep_dense"] = pack_conv_small(dense)
        pk["dep_bias"] = f32(self.dep_proj.bias.detach())
        pk["bins_table"] = f32(wd[:, C:C + D + 1, 0, 0].t())       # row b: dep_proj's column of one-hot channel b
        pk["blocks"] = []
        for blk in list(self.depth_conv)[:3]:
            w1, b1 = _fold(blk.conv1, blk.bn1)
            w2, b2 = _fold(blk.conv2, blk.bn2)
            pk["blocks"].append((pack_conv_small(w1), b1, pack_conv_small(w2), b2))
        if self.use_aspp:
            aspp = self.depth_conv[3]
            pk["aspp"] = []
            for m, dil in zip((aspp.aspp1, aspp.aspp2, aspp.aspp3, aspp.aspp4), ASPP.DILATIONS):
                w, b = _fold(m.atrous_conv, m.bn)
                pk["aspp"].append((pack_conv_small(w), b, w.shape[-1], dil))
            wp, bp = _fold(aspp.global_avg_pool[1], aspp.global_avg_pool[2])
            pk["pool"] = (f32(wp.reshape(C, C).t()), bp)
            wc, bc = _fold(aspp.conv1, aspp.bn1)
            pk["conv1"] = (pack_conv_small(wc[:, :4 * C]), bc, f32(wc[:, 4 * C:, 0, 0].t()))
        final = self.depth_conv[-1]
        pk["final"] = (pack_conv_small(final.weight), f32(final.bias.detach()))
        self._packed = (sig, pk)
        return pk

    def rcs_table(self, rcs_weight, rcs_bias):
        """[(n_rcs + 1), mid]: row 0 = W_r b_E (class -1), row k + 1 = W_r (E[:, k] + b_E) with W_r = dep_proj's columns of the 32
        embedding channels; float64 on the host side of the pack, once per version of the three tensors."""
        sig = tuple((t.data_ptr(), t._version) for t in (rcs_weight, rcs_bias, self.dep_proj.weight))
        if self._tables is None or self._tables[0] != sig:
            C, D = self.mid_channels, self.depth_channels
            wr = self.dep_proj.weight.detach().double()[:, C + D + 1:, 0, 0]                     # [mid, 32]
            e = rcs_weight.detach().double().reshape(rcs_weight.shape[0], -1)                    # [32, n_rcs]
            cols = torch.cat((torch.zeros_like(e[:, :1]), e), dim=1) + rcs_bias.detach().double().view(-1, 1)
            self._tables = (sig, (wr @ cols).t().float().contiguous())
        return self._tables[1]

    def _run_hip(self, x, mlp_input, dense=None, lookup=None):
        pk = self.packed()
        BN, C, H, W = x.shape
        hw, D, ctx, dev = H * W, self.depth_channels, self.context_channels, x.device
        if mlp_input.shape[-1] != 9 or mlp_input.numel() != 9 * BN:
            raise ValueError(f"DepthNet: {BN} maps but mlp_input is {tuple(mlp_input.shape)} (B, N, 9 with B * N maps expected)")
        if dense is not None:
            n_emb = self.dep_proj.weight.shape[1] - C - D - 1
            if tuple(dense[0].shape) != (BN, D + 1, H, W) or tuple(dense[1].shape) != (BN, n_emb, H, W):
                raise ValueError(f"DepthNet: radar_feats [{BN}, {D + 1}, {H}, {W}] and rcs_embedding [{BN}, {n_emb}, {H}, {W}] expected")
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)                        # noqa: E731
        x_rows = pack_rows(x.contiguous(), new(BN, hw, C))
        gates = new(2, BN, C)
        rc = _lib.lib().rac_depthnet_gates_fwd(_lib.ptr(mlp_input.contiguous()), _lib.ptr(pk["gates"]), _lib.ptr(gates), BN, C, 2,
                                               _lib.stream_ptr())
        _lib.check(rc, "rac_depthnet_gates_fwd")
        _note("rac_depthnet_gates_fwd", "2 branches", 2 * BN)
        ld0 = pk["dep_dense"].shape[1] if dense is not None else C
        x0 = conv_small(x_rows, pk["reduce"][0], C, H, W, ksize=3, bias=pk["reduce"][1], relu=True, out=new(BN, hw, ld0))
        out = new(BN, D + ctx, H, W)
        conv_small(x0, pk["context"][0], ctx, H, W, bias=pk["context"][1], gate=gates[0], out=out, channel_first=True, c_off=D)
        if dense is not None:
            radar_feats, rcs_embedding = dense
            pack_rows(radar_feats.contiguous(), x0, c_off=C)
            pack_rows(rcs_embedding.contiguous(), x0, c_off=C + D + 1, c_pad=ld0 - (C + D + 1 + rcs_embedding.shape[1]))
            t = conv_small(x0, pk["dep_dense"], C, H, W, bias=pk["dep_bias"], gate=gates[1])
        else:
            bins, rcs_class, table = lookup
            t = conv_small(x0, pk["dep_x"], C, H, W, bias=pk["dep_bias"], gate=gates[1], bins=bins.contiguous(),
                           bins_table=pk["bins_table"], cls=rcs_class.contiguous(), cls_table=table)
        for w1, b1, w2, b2 in pk["blocks"]:
            u = conv_small(t, w1, C, H, W, ksize=3, bias=b1, relu=True)
            t = conv_small(u, w2, C, H, W, ksize=3, bias=b2, residual=t, relu=True)
        if self.use_aspp:
            img_bias = new(BN, C)
            wp, bp = pk["pool"]
            wc, bc, wb = pk["conv1"]
            rc = _lib.lib().rac_depthnet_pool_bias_fwd(_lib.ptr(t), _lib.ptr(wp), _lib.ptr(bp), _lib.ptr(wb), _lib.ptr(img_bias), BN, hw, C, C,
                                                       C, _lib.stream_ptr())
            _lib.check(rc, "rac_depthnet_pool_bias_fwd")
            _note("rac_depthnet_pool_bias_fwd", "image pool", BN)
            cat = new(BN, hw, 4 * C)
            for i, (w, b, k, dil) in enumerate(pk["aspp"]):
                conv_small(t, w, C, H, W, ksize=k, dilation=dil, bias=b, relu=True, out=cat, c_off=i * C)
            t = conv_small(cat, wc, C, H, W, bias=bc, img_bias=img_bias, relu=True)
        conv_small(t, pk["final"][0], D, H, W, bias=pk["final"][1], out=out, channel_first=True, c_off=0)
        return out

    def forward(self, x, radar_feats, rcs_embedding, mlp_input):
        """x [B*N, C, h, w], radar_feats [B*N, D + 1, h, w], rcs_embedding [B*N, 32, h, w], mlp_input [B, N, 9] ->
        [B*N, D + context, h, w] (depth logits first)."""
        if self.hip_route(x, mlp_input, radar_feats, rcs_embedding):
            with torch.no_grad():
                return self._run_hip(x, mlp_input, dense=(radar_feats, rcs_embedding))
        return self.forward_torch(x, radar_feats, rcs_embedding, mlp_input)

    def forward_fused(self, x, bins, rcs_class, rcs_weight, rcs_bias, mlp_input):
        """The same result from the index maps of ``lss_depth.pool_bins`` (int32 [B*N, h, w]: depth bin 0..D, RCS class -1..) and
        the parameters of ``rcs_embedding``: the prior tensor is never built.  HIP route only (``hip_route`` tells)."""
        if not self.hip_route(x, mlp_input, bins, rcs_class, rcs_weight, rcs_bias):
            raise RuntimeError("DepthNet.forward_fused: not on the HIP route (device float32 tensors, eval(), no gradient, 256 channels, "
                               "BN); call forward() with the dense priors")
        if bins.dtype != torch.int32 or rcs_class.dtype != torch.int32 or bins.shape != rcs_class.shape \
                or tuple(bins.shape) != (x.shape[0],) + tuple(x.shape[2:]):
            raise ValueError("DepthNet.forward_fused: int32 [B*N, h, w] index maps of the feature map's size expected")
        with torch.no_grad():
            return self._run_hip(x, mlp_input, lookup=(bins, rcs_class, self.rcs_table(rcs_weight, rcs_bias)))
