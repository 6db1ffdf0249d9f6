"""The optimiser side of the training recipe (configs/racformer_r50_nuimg_704x256_f8.py:282-305): AdamW with per-parameter learning
rates, gradient clipping at a total 2-norm of 35, cosine annealing with a linear warm-up -- and the step that applies them.

``FusedAdamW``        ``torch.optim.AdamW`` (``amsgrad=False``, ``maximize=False``) with ``clip_grad_norm_(max_norm, norm_type=2)`` folded
                      in.  On device parameters a step is ``rac_adamw_step`` (csrc/optimizer.hip): three launches for all tensors
                      -- sum of squares per chunk, finish, update -- with the norm summed in float64 in a fixed order (same bits every
                      run and wherever the tensors lie), a non-finite norm skipping the whole step on the device (what ``GradScaler.step``
                      does under the reference's ``Fp16OptimizerHook``), no read-back, and ``torch.autograd.graph.increment_version`` on
                      every updated parameter, because the update writes through raw pointers and every weight-derived cache of this
                      package (folded BatchNorms, f16 packs, ``LinearGradPacks``, layer 0's front half, the streaming plan) is keyed on
                      ``(data_ptr, _version)``.  On CPU parameters the same formula in torch ops (float32 or float64): the comparator
                      of the tests and the CPU path.
``build_optimizer``   mmcv 1.6.0's ``DefaultOptimizerConstructor`` for the keys the config uses (``paramwise_cfg.custom_keys`` with
                      ``lr_mult`` / ``decay_mult``).
``CosineAnnealingLr`` mmcv's by-epoch ``CosineAnnealingLrUpdaterHook`` with its iteration-wise warm-up.
``parse_losses`` / ``train_step``  mmdet's ``_parse_losses`` and the order of a training iteration.

Departures from torch / mmcv / mmdet, all deliberate:
  * The clip is folded into the update: ``p.grad`` is read, never written, and stays unclipped.
  * The step is skipped as a whole when the gradients' total norm is not finite (``opt.skipped``); torch would write NaNs.
  * ``opt.grad_norm`` is float64 (the root of the float64 sum of squares); torch's is the float32 norm of float32 norms.
  * ``parse_losses`` keeps ``log_vars`` as detached tensors on the losses' device (no ``.item()``: nothing is read back).
  * ``build_optimizer`` walks ``named_parameters()``, which yields a parameter shared by two modules once (mmcv would list it twice
    and torch refuse the duplicate).
  * A captured step (``torch.cuda.graph``) cannot move ``_version`` on replay: call ``opt.mark_updated()`` after replays before the
    weights are read through a cache.  ``opt.prepare()`` builds the device tables beforehand (an upload cannot be captured), and
    ``sync_hyper()`` -- which the scheduler calls -- carries new learning rates to the device table the captured step reads.
Not here: loss scaling (the package computes in float32; the recipe's scale of 512 is an exact power of two), the EMA hook (the f8
config registers none), data-parallel gradient reduction, weight packs written by the update, zeroing gradients in the kernel."""
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

CHUNK = _lib.OPT_CHUNK
# rac_opt_tensor / rac_opt_chunk (include/racformer_hip.h)
_TENSOR = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i8"), ("row", "<i4"), ("reserved", "<i4")])
_CHUNK = np.dtype([("start", "<i8"), ("tensor", "<i4"), ("reserved", "<i4")])
_ALIGN = 4          # elements: per-tensor views of the flat moment buffers start at multiples of 16 bytes (float32)


def _check_clip(grad_clip):
    if grad_clip is None:
        return None
    extra = set(grad_clip) - {"max_norm", "norm_type"}
    if extra or "max_norm" not in grad_clip:
        raise ValueError(f"FusedAdamW: grad_clip is dict(max_norm=..., norm_type=2) or None, got {grad_clip!r}")
    if float(grad_clip.get("norm_type", 2)) != 2.0:
        raise NotImplementedError(f"FusedAdamW: grad_clip norm_type={grad_clip['norm_type']!r} is not implemented (2 only)")
    max_norm = float(grad_clip["max_norm"])
    if not (max_norm >= 0.0 and math.isfinite(max_norm)):
        raise ValueError(f"FusedAdamW: grad_clip max_norm={max_norm!r} has to be finite and non-negative")
    return max_norm


class FusedAdamW(torch.optim.Optimizer):
    """See the module docstring.  ``self.state[p]`` holds ``step`` (a float32 0-dim view, as torch keeps it), ``exp_avg`` and
    ``exp_avg_sq`` (views of one flat buffer each, starting at 16-byte-aligned offsets) from the first step a parameter takes part in.
    ``grad_norm``, ``grad_norm_sq``, ``clip_coef`` and ``skipped`` are 0-dim tensors on the parameters' device, rewritten by every step
    (the buffers are allocated by the first ``step()`` / ``prepare()`` / ``sync_hyper()``; the attributes exist from then on)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_clip=None, amsgrad=False):
        if amsgrad:
            raise NotImplementedError("FusedAdamW: amsgrad is not implemented")
        if not (lr >= 0.0 and eps >= 0.0 and weight_decay >= 0.0 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdamW: invalid hyper-parameters lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        self.max_norm = _check_clip(grad_clip)
        self._rows = []                 # every parameter of every group, in group order: row r of the per-tensor tables
        self._flat = None               # (exp_avg, exp_avg_sq, steps) flat buffers, offsets per row
        self._signature = None
        self._tables = None
        self._retired = []              # tables a captured graph may still read
        self._hyper_host = None
        self._present = []
        self.table_builds = self.table_uploads = 0      # statistics: tables rebuilt (the structure changed) / gradient pointers re-sent
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False))

    # ---- layout -----------------------------------------------------------------------------------------------------------------
    def add_param_group(self, param_group):
        ps = param_group["params"]
        ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
        for p in ps:
            if p.is_cuda and p.dtype != torch.float32:
                raise ValueError(f"FusedAdamW: device parameters have to be float32, got {p.dtype} (shape {tuple(p.shape)})")
            if p.is_cuda and not p.is_contiguous():
                raise ValueError(f"FusedAdamW: device parameters have to be contiguous (shape {tuple(p.shape)}, strides {p.stride()})")
            if not p.is_cuda and p.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"FusedAdamW: CPU parameters have to be float32 or float64, got {p.dtype}")
        param_group["params"] = ps
        super().add_param_group(param_group)
        g = self.param_groups[-1]
        if g.get("amsgrad") or g.get("maximize"):
            raise NotImplementedError("FusedAdamW: amsgrad / maximize are not implemented")
        self._signature = None

    def _layout(self):
        """The flat buffers and per-row views, (re)built when parameters were added; moments already held are carried over."""
        params = [p for g in self.param_groups for p in g["params"]]
        if self._flat is not None and len(params) == len(self._rows):
            return
        if not params:
            raise ValueError("FusedAdamW: no parameters")
        dev, dtype = params[0].device, params[0].dtype
        if any(p.device != dev or p.dtype != dtype for p in params):
            raise ValueError("FusedAdamW: all parameters have to be on one device and of one dtype")
        offsets, total = [], 0
        for p in params:
            offsets.append(total)
            total += -(-max(p.numel(), 1) // _ALIGN) * _ALIGN
        m, v = torch.zeros(total, dtype=dtype, device=dev), torch.zeros(total, dtype=dtype, device=dev)
        steps = torch.zeros(len(params), dtype=torch.float32, device=dev)
        old = self._flat
        if old is not None:
            n = old[0].numel()
            m[:n], v[:n], steps[:len(self._rows)] = old[0], old[1], old[2]
        self._flat, self._rows = (m, v, steps), params
        self._views = [(m[o:o + p.numel()].view(p.shape), v[o:o + p.numel()].view(p.shape), steps[r]) for r, (p, o) in
                       enumerate(zip(params, offsets))]
        for r, p in enumerate(params):
            if p in self.state:
                self._publish(r)
        if dev.type == "cuda":
            self._hyper_dev = torch.zeros(len(params), _lib.OPT_HYPER, dtype=torch.float64, device=dev)
            self._scalars = torch.zeros(len(params), _lib.OPT_SCALARS, dtype=torch.float32, device=dev)
            # (a page-locked staging copy kept for the purpose, as for the tensor table: see _device_tables)
            self._hyper_stage, self._hyper_sent = torch.zeros(len(params), _lib.OPT_HYPER, dtype=torch.float64).pin_memory(), torch.cuda.Event()
            self._hyper_host = None
        # rac_opt_record: total_sq, total_norm (float64), clip_coef (float32), skip (int32)
        self._record = torch.zeros(3, dtype=torch.float64, device=dev)
        self._record[2:3].view(torch.float32)[0] = 1.0
        self.grad_norm_sq, self.grad_norm = self._record[0], self._record[1]
        self.clip_coef, self.skipped = self._record[2:3].view(torch.float32)[0], self._record[2:3].view(torch.int32)[1]
        self._signature = None

    def _publish(self, row):
        m, v, step = self._views[row]
        self.state[self._rows[row]] = dict(step=step, exp_avg=m, exp_avg_sq=v)

    def _hyper_rows(self):
        rows = []
        for g in self.param_groups:
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError("FusedAdamW: amsgrad / maximize are not implemented")
            b1, b2 = g["betas"]
            rows += [(float(g["lr"]), float(g["weight_decay"]), float(b1), float(b2), float(g["eps"]), 0.0)] * len(g["params"])
        return rows

    def sync_hyper(self):
        """Carries the groups' lr / weight_decay / betas / eps to the device table the finish launch reads: one small copy, and only
        when a value changed.  ``step()`` calls it (not while capturing); a scheduler calls it after writing ``param_groups``."""
        self._layout()
        if self._rows[0].device.type != "cuda":
            return
        rows = self._hyper_rows()
        if rows != self._hyper_host:
            self._hyper_sent.synchronize()
            self._hyper_stage.copy_(torch.tensor(rows, dtype=torch.float64))
            self._hyper_dev.copy_(self._hyper_stage, non_blocking=True)
            self._hyper_sent.record()
            self._hyper_host = rows

    # ---- the step ---------------------------------------------------------------------------------------------------------------
    def _take_part(self):
        """(row, parameter, gradient) of every parameter this step updates: requires_grad and a gradient present, as in torch."""
        out = []
        for r, p in enumerate(self._rows):
            g = p.grad
            if g is None or not p.requires_grad or p.numel() == 0:
                continue
            if g.is_sparse:
                raise RuntimeError("FusedAdamW does not support sparse gradients")
            out.append((r, p, g))
        return out

    def prepare(self):
        """Builds and uploads the tensor and chunk tables for the gradients as they stand now, and the hyper table.  ``step()`` does
        this itself whenever the signature ``(row, parameter pointer, gradient pointer, numel)`` has changed -- except under stream
        capture, where an upload is impossible: call this (or run one eager step) with the gradient buffers in place before capturing."""
        self._layout()
        present = self._take_part()
        if present and present[0][1].is_cuda:
            self._device_tables(present)
            self.sync_hyper()
        return present

    def _device_tables(self, present):
        """The device tables for this step's tensors.  Two signatures: the STRUCTURE (row, parameter pointer, numel per tensor) decides
        the chunk table, the partials and every column of the tensor table but one, and changes when parameters are frozen, added or
        moved; the GRADIENT pointers change every step under ``zero_grad(set_to_none=True)`` (autograd allocates the gradients anew),
        so they take a path that allocates nothing and waits for nothing: the column is rewritten in a page-locked staging copy kept
        for the purpose and sent with one asynchronous 48-byte-per-tensor copy.  (A copy from pageable memory, or page-locked memory
        allocated per step, makes the host wait for the device -- for the whole backward it has just enqueued; DESIGN 3.22c has the
        training-step times of both forms.)"""
        structure = tuple((r, p.data_ptr(), p.numel()) for r, p, _ in present)
        gptrs = [g.data_ptr() for _, _, g in present]
        capturing = torch.cuda.is_current_stream_capturing()
        t = self._tables
        if t is not None and structure == self._signature and gptrs == t["gptrs"]:
            if capturing:
                t["captured"] = True
            return t
        if capturing:
            raise RuntimeError("FusedAdamW.step under stream capture: the parameters / gradient buffers are not the ones the device tables "
                               "were built for; call opt.prepare() (or run one eager step) on these buffers before capturing")
        for r, p, g in present:
            if g.dtype != torch.float32 or g.device != p.device or not g.is_contiguous() or g.shape != p.shape:
                raise ValueError(f"FusedAdamW: the gradient of parameter {r} has to be a contiguous float32 tensor of the parameter's "
                                 f"shape on its device (got {g.dtype}, {tuple(g.shape)}, strides {g.stride()}, {g.device})")
        if t is None or structure != self._signature or t["captured"]:
            t = self._build_tables(present, structure)
        t["sent"].synchronize()                      # (the previous upload has left the staging copy; long since, in practice)
        t["stage_np"]["g"] = gptrs
        t["tensors"].copy_(t["stage"], non_blocking=True)
        t["sent"].record()
        t["gptrs"] = gptrs
        self.table_uploads += 1
        return t

    def _build_tables(self, present, structure):
        for r, p, _ in present:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"FusedAdamW: parameter {r} is no longer a contiguous float32 tensor")
        dev = present[0][1].device
        stage = torch.zeros(len(present) * _TENSOR.itemsize, dtype=torch.uint8).pin_memory()
        tens = stage.numpy().view(_TENSOR)
        chunks = []
        for i, (r, p, _) in enumerate(present):
            m, v, _ = self._views[r]
            tens[i] = (p.data_ptr(), 0, m.data_ptr(), v.data_ptr(), p.numel(), r, 0)
            c = np.zeros(-(-p.numel() // CHUNK), dtype=_CHUNK)
            c["start"] = np.arange(len(c), dtype=np.int64) * CHUNK
            c["tensor"] = i
            chunks.append(c)
        chunks = np.concatenate(chunks)
        assert all(0 <= c["start"] < tens[c["tensor"]]["numel"] for c in chunks[[0, -1]])
        if self._tables is not None and self._tables["captured"]:
            self._retired.append(self._tables)          # (a captured graph holds these addresses: they must not be handed out again)
        self._tables = dict(
            stage=stage, stage_np=tens, sent=torch.cuda.Event(), gptrs=None, tensors=torch.empty(stage.numel(), dtype=torch.uint8, device=dev),
            chunks=torch.from_numpy(chunks.view(np.uint8)).to(dev), partials=torch.zeros(len(chunks), dtype=torch.float64, device=dev),
            n_tensors=len(tens), n_chunks=len(chunks), captured=False)
        self._signature = structure
        self.table_builds += 1
        for r, p, _ in present:
            if p not in self.state:
                self._publish(r)
        return self._tables

    def launch(self, phases=_lib.OPT_ALL):
        """Enqueues the launches named by ``phases`` (``_lib.OPT_NORM | OPT_FINISH | OPT_UPDATE``) on the tables as they stand; for
        ``step()`` and for timing the phases apart (tools/optimizer_bench.py)."""
        t = self._tables
        _lib.check(_lib.lib().rac_adamw_step(
            _lib.ptr(t["tensors"]), t["n_tensors"], _lib.ptr(t["chunks"]), t["n_chunks"], _lib.ptr(self._hyper_dev), _lib.ptr(self._flat[2]),
            _lib.ptr(self._scalars), _lib.ptr(t["partials"]), _lib.ptr(self._record), -1.0 if self.max_norm is None else self.max_norm,
            phases, _lib.stream_ptr()), "rac_adamw_step")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._layout()
        present = self._take_part()
        if not present:
            return loss
        self._present = [p for _, p, _ in present]
        if present[0][1].is_cuda:
            _lib.lib()
            self._device_tables(present)
            if not torch.cuda.is_current_stream_capturing():
                self.sync_hyper()
            self.launch()
            self.mark_updated()
        else:
            self._step_torch(present)
        return loss

    def mark_updated(self):
        """``_version`` + 1 on the parameters of the last step: the kernels write through raw pointers, and the package's weight caches
        are keyed on the version.  ``step()`` calls it; after replaying a captured step the caller does."""
        if self._present:
            torch.autograd.graph.increment_version(self._present)

    def _step_torch(self, present):
        """The kernel's formula in torch ops, in the parameters' dtype; the per-tensor scalars in float64 as there, the norm in float64
        composed as ``clip_grad_norm_`` composes it (the library's norm per tensor, then the norm of those: on float64 parameters the very
        value torch clips by, which is a few 1e-15 off the exactly rounded root the kernels' fixed tree stays within)."""
        norm = float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g, 2, dtype=torch.float64) for _, _, g in present]), 2))
        total = norm * norm
        finite = math.isfinite(total)
        coef = 1.0 if self.max_norm is None or not finite else min(1.0, self.max_norm / (norm + 1e-6))
        self._record[0], self._record[1] = total, norm
        self._record[2:3].view(torch.float32)[0] = coef
        self._record[2:3].view(torch.int32)[1] = 0 if finite else 1
        if not finite:
            return
        hyper = self._hyper_rows()
        for r, p, g in present:
            if p not in self.state:
                self._publish(r)
            m, v, step = self._views[r]
            lr, wd, b1, b2, eps, _ = hyper[r]
            step += 1
            t = float(step)
            gc = g * coef
            p.mul_(1.0 - lr * wd)
            m.add_((gc - m) * (1.0 - b1))
            v.mul_(b2).add_(((1.0 - b2) * gc) * gc)
            p.sub_((lr / (1.0 - b1 ** t)) * (m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)))

    # ---- torch.optim.AdamW's state dict -----------------------------------------------------------------------------------------
    def state_dict(self):
        """``torch.optim.AdamW``'s format: per-parameter ``step`` (a CPU float32 0-dim tensor: the counters are read back here),
        ``exp_avg``, ``exp_avg_sq`` (copies, not views of the flat buffers), and ``param_groups``."""
        sd = super().state_dict()
        sd["state"] = {k: dict(step=s["step"].detach().cpu().clone(), exp_avg=s["exp_avg"].detach().clone(),
                               exp_avg_sq=s["exp_avg_sq"].detach().clone()) for k, s in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """Accepts a state dict of this class or of ``torch.optim.AdamW`` (``amsgrad=False``, ``maximize=False``): the moments are
        copied into the flat buffers, the step counters into the device counters."""
        for g in state_dict["param_groups"]:
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError("FusedAdamW.load_state_dict: amsgrad / maximize states are not implemented")
            if g.get("decoupled_weight_decay") is False:
                raise NotImplementedError("FusedAdamW.load_state_dict: this is torch.optim.Adam's state (weight decay as L2), not AdamW's")
        super().load_state_dict(state_dict)
        loaded = dict(self.state)
        self._flat = None
        self._rows = []
        self.state.clear()
        self._layout()
        with torch.no_grad():
            for r, p in enumerate(self._rows):
                s = loaded.get(p)
                if s is None:
                    continue
                m, v, step = self._views[r]
                m.copy_(s["exp_avg"])
                v.copy_(s["exp_avg_sq"])
                step.copy_(torch.as_tensor(s["step"], dtype=torch.float32))
                self._publish(r)


def build_optimizer(model, cfg):
    """mmcv 1.6.0's ``build_optimizer`` + ``DefaultOptimizerConstructor`` for the recipe's keys:
    ``dict(type='AdamW', lr=..., weight_decay=..., betas=..., eps=..., paramwise_cfg=dict(custom_keys={key: dict(lr_mult=, decay_mult=)}))``
    and, beside them, ``grad_clip`` (the recipe's ``optimizer_config['grad_clip']``).  With a ``paramwise_cfg`` each parameter is its
    own group; the keys are sorted alphabetically, then by length with the longest first, and the first that is a substring of the
    parameter's full name sets ``lr = base * lr_mult`` and ``weight_decay = base * decay_mult`` (both default 1); a frozen parameter's
    group carries no override.  Without ``paramwise_cfg``: one group of all parameters."""
    cfg = dict(cfg)
    if cfg.pop("type", "AdamW") != "AdamW":
        raise NotImplementedError("build_optimizer: only type='AdamW' is implemented")
    paramwise = cfg.pop("paramwise_cfg", None)
    grad_clip = cfg.pop("grad_clip", None)
    base_lr, base_wd = cfg.get("lr"), cfg.get("weight_decay")
    if base_lr is None:
        raise ValueError("build_optimizer: cfg needs 'lr'")
    if paramwise is None:
        return FusedAdamW(list(model.parameters()), grad_clip=grad_clip, **cfg)
    extra = set(paramwise) - {"custom_keys"}
    if extra:
        raise NotImplementedError(f"build_optimizer: paramwise_cfg keys {sorted(extra)} are not implemented (custom_keys only)")
    custom = paramwise.get("custom_keys", {})
    for key, val in custom.items():
        if set(val) - {"lr_mult", "decay_mult"}:
            raise NotImplementedError(f"build_optimizer: custom key {key!r}: only lr_mult / decay_mult are implemented, got {sorted(val)}")
    keys = sorted(sorted(custom), key=len, reverse=True)
    groups = []
    for name, p in model.named_parameters():
        group = dict(params=[p])
        if p.requires_grad:
            for key in keys:
                if key in name:
                    group["lr"] = base_lr * custom[key].get("lr_mult", 1.0)
                    if base_wd is not None:
                        group["weight_decay"] = base_wd * custom[key].get("decay_mult", 1.0)
                    break
        groups.append(group)
    return FusedAdamW(groups, grad_clip=grad_clip, **cfg)


class CosineAnnealingLr:
    """mmcv 1.6.0's ``CosineAnnealingLrUpdaterHook`` run by epoch, with its iteration-wise warm-up (``lr_config`` of the recipe).  The
    training loop calls ``before_train_epoch(epoch)`` at the start of every epoch and ``before_train_iter(cur_iter)`` (the global
    iteration count) before every iteration, as the runner calls the hook:
        regular_g(epoch) = end_g + 0.5 (base_g - end_g)(cos(pi epoch / max_epochs) + 1),   end_g = base_g min_lr_ratio
        cur_iter < warmup_iters:  lr_g = regular_g (1 - (1 - cur_iter / warmup_iters)(1 - warmup_ratio))
        cur_iter == warmup_iters: lr_g = regular_g;   later iterations leave what the epoch set
    ``base_g`` is each group's ``initial_lr`` (its ``lr`` at construction), so ``lr_mult`` carries through.  After writing
    ``param_groups`` it calls ``optimizer.sync_hyper()`` where the optimiser has one: one small copy when a value changed."""

    def __init__(self, optimizer, max_epochs, warmup="linear", warmup_iters=500, warmup_ratio=1.0 / 3, min_lr_ratio=1e-3):
        if warmup not in (None, "linear"):
            raise NotImplementedError(f"CosineAnnealingLr: warmup={warmup!r} is not implemented (None or 'linear')")
        if warmup is not None and not (warmup_iters > 0 and 0 < warmup_ratio <= 1.0):
            raise ValueError("CosineAnnealingLr: warmup_iters has to be positive and warmup_ratio in (0, 1]")
        self.optimizer, self.max_epochs, self.warmup = optimizer, max_epochs, warmup
        self.warmup_iters, self.warmup_ratio, self.min_lr_ratio = warmup_iters, warmup_ratio, min_lr_ratio
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self.base_lr = [g["initial_lr"] for g in optimizer.param_groups]
        self.regular_lr = list(self.base_lr)

    def get_regular_lr(self, epoch):
        out = []
        for base in self.base_lr:
            end = base * self.min_lr_ratio
            out.append(end + 0.5 * (base - end) * (math.cos(math.pi * (epoch / self.max_epochs)) + 1))
        return out

    def get_warmup_lr(self, cur_iter):
        k = (1 - cur_iter / self.warmup_iters) * (1 - self.warmup_ratio)
        return [lr * (1 - k) for lr in self.regular_lr]

    def _set_lr(self, lrs):
        for g, lr in zip(self.optimizer.param_groups, lrs):
            g["lr"] = lr
        sync = getattr(self.optimizer, "sync_hyper", None)
        if sync is not None:
            sync()

    def before_train_epoch(self, epoch):
        self.regular_lr = self.get_regular_lr(epoch)
        self._set_lr(self.regular_lr)

    def before_train_iter(self, cur_iter):
        if self.warmup is None or cur_iter > self.warmup_iters:
            return
        if cur_iter == self.warmup_iters:
            self._set_lr(self.regular_lr)
        else:
            self._set_lr(self.get_warmup_lr(cur_iter))


def parse_losses(losses):
    """mmdet's ``BaseDetector._parse_losses``: every entry reduced to its mean (a list of tensors to the sum of their means); the total is
    the sum of the entries whose key contains ``loss``.  Returns ``(loss, log_vars)`` with ``log_vars['loss']`` the total; the values of
    ``log_vars`` are detached tensors on the losses' device (departure: mmdet calls ``.item()`` on each)."""
    log_vars = OrderedDict()
    for name, value in losses.items():
        if isinstance(value, torch.Tensor):
            log_vars[name] = value.mean()
        elif isinstance(value, list):
            log_vars[name] = sum(v.mean() for v in value)
        else:
            raise TypeError(f"{name} is not a tensor or list of tensors")
    loss = sum(v for k, v in log_vars.items() if "loss" in k)
    log_vars["loss"] = loss
    return loss, OrderedDict((k, v.detach()) for k, v in log_vars.items())


def train_step(model, optimizer, **data):
    """One training iteration in the order of mmcv's runner and optimizer hook: gradients dropped (``set_to_none``), the model's losses
    (``model(return_loss=True, **data)``), their total, backward, ``optimizer.step()`` (the clip is inside it).  Returns ``log_vars``."""
    optimizer.zero_grad(set_to_none=True)
    losses = model(return_loss=True, **data)
    loss, log_vars = parse_losses(losses)
    loss.backward()
    optimizer.step()
    return log_vars
