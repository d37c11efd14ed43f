"""The pipelined, mode-specialised Winograd output transform (ops/csrc/winograd_f32.hip
``k_wg_output_p``, ``EWDML_WG_OUT_PIPE=1`` / ``wg_set_out_pipe(1)``) against the general kernel
(``k_wg_output``, ``wg_set_out_pipe(0)``), on the same inputs.  The default (2) runs the
pipelined kernel only for the instances measured faster in a step.

The new kernel keeps the grid, the thread-to-(tile, channel) mapping, each thread's tile order,
the accumulation order and the expressions, so ``y`` and the whole BN partial-sum buffer must be
bitwise equal: the comparison is on the bit patterns (NaNs included), no tolerance.  Shapes are
the smallest that reach each way the tile loop can go: a thread with one tile (no prefetch), with
several (prologue, steady state, drain), row groups with no tile at all, the divergent last pass
at 64 channels (two row groups in one wave), both vector widths, both tile sizes and every
instantiated epilogue mode.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


@pytest.fixture(scope="module")
def C_():
    from ewdml import ops

    return ops.require()


@pytest.fixture(autouse=True)
def _restore_switch(C_):
    prev = C_.wg_set_out_pipe(-1)
    yield
    C_.wg_set_out_pipe(prev)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _inputs(m, N, H, W, Nc, stat, res, add, seed=0):
    """Random normal operands of one output-transform call.  stat: none / fwd / bwd / bwdc."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=g)

    tiles = N * (H // m) * (W // m)
    d = {"Mo": rn((m + 2) ** 2 * tiles * Nc), "tiles": tiles}
    d["addend"] = rn(N * H * W * Nc) if add else None
    d["h"] = d["res"] = d["code"] = d["stats"] = None
    if stat in ("bwd", "bwdc"):
        s = 2 if stat == "bwdc" else 1  # h is the pool's input: 2H x 2W
        rows = N * H * s * W * s
        h = rn(rows, Nc)
        stats = rn(4, Nc)
        # relu'(h * scale + shift) at exactly 0 (masked: z <= 0) and at NaN (kept: !(z <= 0)):
        # channels 0..3 get shift 0, a few of their h entries 0 and NaN
        stats[3, :4] = 0.0
        h[0:rows:5, 0] = 0.0
        h[1:rows:7, 1] = float("nan")
        h[2:rows:3, 2] = 0.0
        h[0:rows:4, 3] = float("nan")
        d["h"], d["stats"] = h, stats
        if res:
            d["res"] = rn(rows, Nc)
            d["res"][0:rows:5, 0] = 0.0  # keeps z at exactly 0 there
        if stat == "bwdc":
            d["code"] = torch.randint(0, 4, (N * H * W, Nc), device="cuda", generator=g,
                                      dtype=torch.uint8)
    return d


def _run(C_, on, m, N, H, W, Nc, stat, relu, tpb, d):
    C_.wg_set_out_pipe(on)
    y = torch.full((N * H * W * Nc,), SENTINEL, device="cuda")
    part = None
    if stat != "none":
        part = torch.full((2 * d["tiles"] * Nc + 64,), SENTINEL, device="cuda")
    rows = C_.wino_f32_output(_ptr(d["Mo"]), _ptr(y), N, H, W, Nc, m, _ptr(d["h"]),
                              _ptr(d["res"]), _ptr(d["code"]), _ptr(d["stats"]), int(relu),
                              _ptr(part), 0 if part is None else part.numel(),
                              _ptr(d["addend"]), tpb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y, part, rows


def _check(C_, m, N, H, W, Nc, stat, res, relu, add, tpb, seed=0):
    d = _inputs(m, N, H, W, Nc, stat, res, add, seed)
    y0, p0, r0 = _run(C_, 0, m, N, H, W, Nc, stat, relu, tpb, d)
    y1, p1, r1 = _run(C_, 1, m, N, H, W, Nc, stat, relu, tpb, d)
    assert r0 == r1
    assert (y0 != SENTINEL).all()  # every output written (the old kernel's, so the new one's)
    assert torch.equal(y1.view(torch.int32), y0.view(torch.int32))
    if stat == "none":
        assert r0 == 0
        return
    vw = 2 if Nc <= 512 else 4
    rpi = 256 // (Nc // vw)
    want = -(-d["tiles"] // (tpb if tpb else rpi))
    assert r0 == want
    assert torch.equal(p1.view(torch.int32), p0.view(torch.int32))
    assert (p0[2 * r0 * Nc:] == SENTINEL).all()  # nothing past the rows returned
    if stat == "bwd" or stat == "bwdc":
        assert torch.isnan(p0[:2 * r0 * Nc]).any()  # the NaN probes reached the sums


# (m, N, H, W, Nc, tpb): the loop shapes
LOOPS = [
    pytest.param(2, 2, 4, 4, 512, 1, id="one-tile-per-thread"),       # no next tile to prefetch
    pytest.param(2, 2, 4, 4, 512, 3, id="three-tiles-short-last"),    # prologue, steady, drain
    pytest.param(2, 2, 4, 4, 512, 8, id="eight-tiles-one-block"),     # both register sets, 4 rounds
    pytest.param(2, 3, 6, 6, 128, 0, id="rpi4-plan-short-last-block"),  # 27 tiles, 4 per block
    pytest.param(2, 3, 6, 6, 128, 6, id="rpi4-tpb6"),    # tpb no multiple of rpi; groups 1 or 2 tiles
    pytest.param(2, 3, 6, 6, 128, 10, id="rpi4-tpb10"),  # last block: 7 tiles, a group with one
    pytest.param(2, 3, 6, 6, 128, 1, id="rpi4-tpb1"),    # row groups 1..3 get no tile: zero sums
    pytest.param(2, 4, 4, 4, 64, 12, id="nc64-divergent-last-pass"),  # two row groups per wave
    pytest.param(2, 1, 4, 4, 1024, 1, id="vw4-one-tile"),
    pytest.param(2, 1, 4, 4, 1024, 3, id="vw4-three-tiles"),
    pytest.param(4, 2, 8, 8, 128, 6, id="m4-rpi4-tpb6"),
    pytest.param(4, 1, 8, 8, 512, 3, id="m4-three-tiles"),
]


@pytest.mark.parametrize("m,N,H,W,Nc,tpb", LOOPS)
@pytest.mark.parametrize("stat,relu", [("fwd", 0), ("bwd", 1)])
def test_tile_loop_shapes_bitwise(C_, m, N, H, W, Nc, tpb, stat, relu):
    _check(C_, m, N, H, W, Nc, stat, False, relu, False, tpb)


# (stat, res, relu, add): every instantiated epilogue
MODES = [("none", 0, 0, 0), ("none", 0, 0, 1), ("fwd", 0, 0, 0)]
MODES += [("bwd", r, u, a) for r in (0, 1) for u in (0, 1) for a in (0, 1)]
MODES += [("bwdc", 0, 0, 0), ("bwdc", 0, 1, 0)]


@pytest.mark.parametrize("stat,res,relu,add", MODES)
@pytest.mark.parametrize("m,N,H,W,Nc,tpb", [
    pytest.param(2, 3, 6, 6, 128, 6, id="m2-vw2"),
    pytest.param(2, 1, 4, 4, 1024, 3, id="m2-vw4"),
    pytest.param(4, 2, 8, 8, 128, 6, id="m4-vw2"),
])
def test_every_mode_bitwise(C_, m, N, H, W, Nc, tpb, stat, res, relu, add):
    if stat == "none":
        tpb = 0  # without partial sums the plan's one pass per block
    _check(C_, m, N, H, W, Nc, stat, bool(res), relu, bool(add), tpb, seed=1)


@pytest.mark.parametrize("m,Nc,stat,res,add", [
    pytest.param(2, 128, "bwdc", 1, 0, id="pool-codes-with-residual"),
    pytest.param(2, 128, "bwdc", 0, 1, id="pool-codes-with-addend"),
    pytest.param(2, 128, "fwd", 0, 1, id="forward-statistics-with-addend"),
    pytest.param(4, 1024, "fwd", 0, 0, id="m4-vw4"),
])
def test_uninstantiated_combination_raises(C_, m, Nc, stat, res, add):
    N, H, W = 1, 8, 8
    d = _inputs(m, N, H, W, Nc, stat, bool(res), bool(add))
    with pytest.raises(RuntimeError, match="no pipelined kernel"):
        _run(C_, 1, m, N, H, W, Nc, stat, 1, 0, d)
    y0, p0, _ = _run(C_, 0, m, N, H, W, Nc, stat, 1, 0, d)  # the general kernel takes it
    y2, p2, _ = _run(C_, 2, m, N, H, W, Nc, stat, 1, 0, d)  # and so does the default
    assert torch.equal(y2.view(torch.int32), y0.view(torch.int32))
    assert torch.equal(p2.view(torch.int32), p0.view(torch.int32))


def test_default_takes_measured_instances_only(C_):
    """Mode 2 (the default without EWDML_WG_OUT_PIPE) is what a fresh process runs; every mode of
    the switch gives the same bits on a measured instance (m = 2, forward sums) and on one the
    default leaves to the general kernel (m = 4)."""
    import os

    if os.environ.get("EWDML_WG_OUT_PIPE") is None:
        assert C_.wg_set_out_pipe(-1) == 2
    for m, N, H, W, Nc in ((2, 3, 6, 6, 128), (4, 2, 8, 8, 128)):
        d = _inputs(m, N, H, W, Nc, "fwd", False, False, seed=2)
        outs = [_run(C_, on, m, N, H, W, Nc, "fwd", 0, 6, d) for on in (0, 1, 2)]
        for y, p, r in outs[1:]:
            assert r == outs[0][2]
            assert torch.equal(y.view(torch.int32), outs[0][0].view(torch.int32))
            assert torch.equal(p.view(torch.int32), outs[0][1].view(torch.int32))
