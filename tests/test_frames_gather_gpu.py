"""rac_frames_gather (csrc/frames.hip) on the device: every case bitwise against torch.index_select, with canary elements in front of
and behind every ``out`` left untouched."""
import pytest
import torch

from racformer_amd import fused, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64              # float32 elements (256 bytes) on either side of an out
PIECE = 4096             # 16-byte units a workgroup moves per pass (256 lanes x 4)


def make(frame_units, n_slots, T, seed):
    """(ring [n_slots, units * 4] float32 of distinct bit patterns, padded out buffer, its view [T, units * 4])"""
    g = torch.Generator().manual_seed(seed)
    ring = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_slots, frame_units * 4), dtype=torch.int32, generator=g).view(torch.float32).to(DEV)
    buf = torch.full((2 * CANARY + T * frame_units * 4,), -7.25, dtype=torch.float32, device=DEV)
    return ring, buf, buf[CANARY:CANARY + T * frame_units * 4].view(T, frame_units * 4)


def check(rings, bufs, outs, slots):
    idx = torch.tensor(slots, device=DEV)
    for ring, buf, out in zip(rings, bufs, outs):
        want = torch.index_select(ring, 0, idx)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        assert bool((buf[:CANARY] == -7.25).all()) and bool((buf[-CANARY:] == -7.25).all())


@pytest.mark.parametrize("units", [1, 257, PIECE * 3 + 1])
@pytest.mark.parametrize("T", [1, 3, 16])
def test_one_tensor_sizes_and_tails(units, T):
    n_slots = 19
    ring, buf, out = make(units, n_slots, T, units + T)
    slots = [(7 * t + 3) % n_slots for t in range(T)]
    fused.frames_gather([ring], [out], slots)
    torch.cuda.synchronize()
    check([ring], [buf], [out], slots)


def test_repeated_slots_and_identity():
    ring, buf, out = make(PIECE + 5, 16, 16, 1)
    for slots in ([5] * 16, [0, 0, 15, 15, 3, 3, 3, 9, 0, 15, 1, 1, 2, 2, 2, 2], list(range(16))):
        buf[CANARY:-CANARY] = 0
        fused.frames_gather([ring], [out], slots)
        torch.cuda.synchronize()
        check([ring], [buf], [out], slots)


def test_six_unequal_tensors_in_one_launch():
    """The split of the workgroups among tensors of very different sizes: a tensor of one unit beside one of 12 pieces and a tail."""
    T, n_slots = 3, 18
    sizes = [PIECE * 12 + 3, 1, 257, PIECE * 2, 16, PIECE - 1]
    made = [make(u, n_slots, T, 10 + i) for i, u in enumerate(sizes)]
    rings, bufs, outs = [m[0] for m in made], [m[1] for m in made], [m[2] for m in made]
    slots = [17, 0, 17]
    fused.frames_gather(rings, outs, slots)
    torch.cuda.synchronize()
    check(rings, bufs, outs, slots)


def test_small_pyramid_tensors_twice_and_captured():
    """The six tensors of the detector's memory at synthetic.SMALL ([G, N, H, W, 64] per level, [256, 16, 16] BEV maps): two runs
    give the same bits, and a captured launch replays them into buffers filled with something else in between."""
    cfg = syn.SMALL
    T, n_slots = cfg.num_frames, 15 + cfg.num_frames
    shapes = [(4, cfg.num_cams, h, w, 64) for h, w in cfg.fpn_hw] + [(256,) + tuple(cfg.bev_hw)] * 2
    rings = [torch.randn((n_slots,) + s, device=DEV) for s in shapes]
    bufs = [torch.full((2 * CANARY + T * r[0].numel(),), -7.25, device=DEV) for r in rings]
    outs = [b[CANARY:-CANARY].view((T * s[0],) + s[1:]) if i < 4 else b[CANARY:-CANARY].view((1, T) + s)
            for i, (b, s) in enumerate(zip(bufs, shapes))]
    slots = [4, 17, 4]
    flat = [o.view(T, -1) for o in outs]
    fused.frames_gather(rings, outs, slots)
    torch.cuda.synchronize()
    check([r.view(n_slots, -1) for r in rings], bufs, flat, slots)
    first = [o.clone() for o in outs]
    fused.frames_gather(rings, outs, slots)
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, outs))
    # captured: the slot table is part of the captured launch's arguments
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused.frames_gather(rings, outs, slots)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused.frames_gather(rings, outs, slots)
    for o in outs:
        o.zero_()
    graph.replay()
    torch.cuda.synchronize()
    check([r.view(n_slots, -1) for r in rings], bufs, flat, slots)
    for r in rings:
        r.mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    check([r.view(n_slots, -1) for r in rings], bufs, flat, slots)
