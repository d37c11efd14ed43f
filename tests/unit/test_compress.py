"""Codec semantics on the torch oracle: exact top-k, QSGD unbiasedness, zero guards, payload
sizes and the reference-equivalent byte figures of BASELINE.md / SURVEY section 6.1."""
import numpy as np
import pytest
import torch

from ewdml.compress import QSGDCompressor, TopKCompressor, TopKQSGDCompressor, oracle, rng
from ewdml.compress.plan import CHUNK, BucketPlan, Layout
from ewdml.models import build_model
from ewdml.parallel.flat import FlatModel


def _plan(numels, ratio=0.01):
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(numels, offs, ratio, 0, o)


def test_rng_matches_python_int_reference():
    idx = torch.tensor([0, 1, 2, 12345, 2 ** 31 + 7, 2 ** 32 - 1])
    key = rng.stream_key(5, 17, 3)
    got = rng.mix32(idx ^ key)
    exp = [rng.mix32_int(int(i) ^ key) for i in idx]
    assert got.tolist() == exp
    u = rng.uniform(torch.arange(100000), key)
    assert 0 <= float(u.min()) and float(u.max()) < 1
    assert abs(float(u.mean()) - 0.5) < 0.01


def test_topk_indices_exact_and_sorted():
    g = torch.Generator().manual_seed(0)
    for n, k in [(10, 1), (1000, 10), (100000, 1000), (5, 5)]:
        x = torch.randn(n, generator=g)
        idx = oracle.topk_indices(x, k)
        assert idx.numel() == k
        assert torch.all(idx[1:] > idx[:-1])
        ref = torch.topk(x.abs(), k).values
        torch.testing.assert_close(x[idx].abs().sort().values, ref.sort().values)


def test_topk_ties_lowest_index():
    x = torch.tensor([1.0, -2.0, 2.0, 2.0, 0.5, -2.0])
    idx = oracle.topk_indices(x, 2)
    assert idx.tolist() == [1, 2]


def test_qsgd_unbiased_and_bounded():
    x = torch.randn(2000)
    acc = torch.zeros_like(x)
    trials = 400
    scale = float(x.abs().max())
    for t in range(trials):
        q = oracle.quantize(x, scale, 7, torch.arange(x.numel()), rng.stream_key(0, t, 0))
        assert int(q.abs().max()) <= 7
        acc += q.float() * oracle.dequant_step(7, scale)
    err = (acc / trials - x).abs().max()
    assert err < 0.2 * scale / 7 * 3  # ~3 sigma of the mean of 400 Bernoulli roundings


def test_zero_gradient_gives_zero_not_nan():
    plan = _plan([100, 7])
    for kind in ("topk_qsgd", "qsgd"):
        lay = Layout.build(kind, plan, 8)
        g = torch.zeros(plan.length)
        enc = oracle.encode_topk if kind != "qsgd" else oracle.encode_qsgd
        pay = enc(g, plan, lay, 127, "l2", 0)
        dec = oracle.decode_sum(pay[None], plan, lay, 127, 1.0)
        assert torch.isfinite(dec).all() and float(dec.abs().sum()) == 0.0


@pytest.mark.parametrize("kind,bits", [("topk_qsgd", 8), ("topk_qsgd", 4), ("topk", 8),
                                       ("qsgd", 8), ("qsgd", 4)])
def test_roundtrip_recovers_selected_values(kind, bits):
    plan = _plan([CHUNK * 2 + 11, 33, 500], 0.05)
    lay = Layout.build(kind, plan, bits)
    levels = 127 if bits == 8 else 7
    g = torch.randn(plan.length)
    enc = oracle.encode_qsgd if kind == "qsgd" else oracle.encode_topk
    pay = enc(g.clone(), plan, lay, levels, "max", 1)
    assert pay.numel() == lay.nbytes
    dec = oracle.decode_sum(pay[None], plan, lay, levels, 1.0)
    for off, n, k in zip(plan.offsets, plan.numels, plan.ks):
        x, d = g[off:off + n], dec[off:off + n]
        if kind == "qsgd":
            assert (d - x).abs().max() <= x.abs().max() / levels * 1.0001
        else:
            sel = oracle.topk_indices(x, k)
            mask = torch.zeros(n, dtype=torch.bool)
            mask[sel] = True
            assert float(d[~mask].abs().sum()) == 0.0
            tol = 0 if kind == "topk" else float(x.abs().max()) / levels * 1.0001
            assert (d[mask] - x[mask]).abs().max() <= tol


def test_error_feedback_residual_is_untransmitted_part():
    plan = _plan([3000], 0.01)
    lay = Layout.build("topk_qsgd", plan, 8)
    g = torch.randn(plan.length)
    r = torch.zeros(plan.length)
    pay = oracle.encode_topk(g.clone(), plan, lay, 127, "max", 3, residual=r)
    dec = oracle.decode_sum(pay[None], plan, lay, 127, 1.0)
    torch.testing.assert_close(dec[:3000] + r[:3000], g[:3000], rtol=0, atol=1e-6)


def test_vgg11_payload_reaches_100x():
    """VGG-11 top-1 % + int8 + u16 segment indices -> ~0.28 MiB/worker, >=100x."""
    flat = FlatModel(build_model("VGG11"), bucket_bytes=1 << 40)
    plan = BucketPlan(flat.buckets[0].plan.numels, flat.buckets[0].plan.offsets, 0.01, 0,
                      flat.buckets[0].plan.length)
    assert plan.total_k == 97555
    lay = Layout.build("topk_qsgd", plan, 8)
    dense = 9756426 * 4
    assert lay.nbytes / 2 ** 20 < 0.29
    ratio = dense / lay.nbytes
    assert ratio > 130  # reference-equivalent 148.87 MiB -> 4 * payload
    # reference-equivalent per-step MiB (2 workers x push+pull) below the report's 1.48 MB
    assert 4 * lay.nbytes / 2 ** 20 < 1.48
    lay4 = Layout.build("topk_qsgd", plan, 4)
    assert dense / lay4.nbytes > 155


def test_lenet_payload():
    flat = FlatModel(build_model("LeNet"), bucket_bytes=1 << 40)
    p = flat.buckets[0].plan
    plan = BucketPlan(p.numels, p.offsets, 0.01, 0, p.length)
    assert plan.total_k == 4313
    lay = Layout.build("topk_qsgd", plan, 8)
    assert 431080 * 4 / lay.nbytes > 125
    assert 4 * lay.nbytes / 2 ** 20 < 0.066  # report Method 6 figure for LeNet


def test_reference_method_byte_model():
    """Methods 1/3 = 4D, 4 = D (8-bit), 5 = 0.8D (K=0.4, 1 B value + 1 B index)."""
    D = 9756426 * 4 / 2 ** 20
    assert abs(4 * D - 148.87) < 0.01
    assert abs(D - 37.22) < 0.01


def test_reference_api_notebook_examples():
    # QSGD and topk Sparsification.ipynb#cell0: s=64 round trip of a 3-element tensor
    q = QSGDCompressor(quantum_num=64)
    t = torch.tensor([0.01, 0.01, 1.0])
    levels, norm = q.compress(t)
    assert levels.dtype == torch.int8 and levels.shape == t.shape
    assert int(levels[2]) == 64  # the spike quantises to the top level (the notebook prints 128.
    dec = q.decompress((levels, norm))  # with s=128; here s=64 fits int8)
    assert abs(float(dec[2]) - 1.0) < 0.02
    # Horovod-style signature decompress(levels, ctx=norm)
    torch.testing.assert_close(q.decompress(levels, norm), dec)
    # cell2: TopK 0.4 on a 4x3 tensor -> k = 4
    tk = TopKCompressor(0.4)
    x = torch.arange(12, dtype=torch.float32).view(4, 3) - 6
    (vals, idx), ctx = tk.compress(x)
    assert vals.numel() == 4 and ctx == (12, x.size())
    back = tk.decompress((vals, idx), ctx)
    assert back.shape == x.shape and int((back != 0).sum()) == 4
    c = TopKQSGDCompressor(0.5)
    out, ctx = c.compress(torch.randn(100))
    assert c.decompress(out, ctx).shape == (100,)


def test_fp32_step_rounding_consistency():
    # dequant step is fp32(scale) * fp32(1/levels), exactly as the kernels compute it
    s = oracle.dequant_step(127, 0.3)
    assert s == float(np.float32(0.3) * np.float32(1 / 127))
    assert oracle.inv_scale(127, 0.0) == 0.0


def test_dgc_conservation_and_masking():
    """Momentum-corrected error feedback (oracle.dgc_accumulate): what is sent plus the new
    residual equals the old residual plus the velocity step, and the velocity is zero exactly at
    the sent coordinates (momentum factor masking)."""
    plan = _plan([3000, 700], 0.02)
    lay = Layout.build("topk", plan, 8)
    gen = torch.Generator().manual_seed(0)
    r = torch.zeros(plan.length)
    u = torch.zeros(plan.length)
    for step in range(4):
        g = torch.randn(plan.length, generator=gen)
        r_old, u_old = r.clone(), u.clone()
        pay = oracle.encode_topk(g.clone(), plan, lay, 127, "max", step, residual=r,
                                 dgc=dict(velocity=u, momentum=0.9))
        sent = oracle.decode_sum(pay[None], plan, lay, 127, 1.0)
        u_new = u_old * 0.9 + g
        e = r_old + u_new
        torch.testing.assert_close(sent + r, e, rtol=0, atol=0)  # plain top-k: exact values
        mask = sent != 0
        assert int(mask.sum()) == plan.total_k
        assert torch.equal(u[mask], torch.zeros(int(mask.sum())))
        assert torch.equal(u[~mask], u_new[~mask])


def test_dgc_without_momentum_is_plain_error_feedback():
    plan = _plan([5000], 0.01)
    lay = Layout.build("topk_qsgd", plan, 8)
    g = torch.randn(plan.length)
    r1, r2, u = torch.randn(plan.length) * 0.1, None, torch.zeros(plan.length)
    r2 = r1.clone()
    a = oracle.encode_topk(g.clone(), plan, lay, 127, "max", 5, residual=r1)
    b = oracle.encode_topk(g.clone(), plan, lay, 127, "max", 5, residual=r2,
                           dgc=dict(velocity=u, momentum=0.0))
    assert torch.equal(a, b) and torch.equal(r1, r2)


def test_dense_below_sends_small_tensors_whole():
    plan = BucketPlan([64, 64, 100000], [0, 64, 128], 0.01, dense_below=64)
    assert plan.ks == [64, 64, 1000]
    assert plan.tensor_bm0[:2] == [0, 2] and plan.tensor_bm0[2] == -1  # whole: bitmap-indexed
    lay = Layout.build("topk", plan, 8)
    g = torch.randn(plan.length)
    pay = oracle.encode_topk(g, plan, lay, 127, "max", 1)
    dec = oracle.decode_sum(pay[None], plan, lay, 127, 1.0)
    assert torch.equal(dec[:128], g[:128])


@pytest.mark.parametrize("kind,bits", [("topk", 8), ("topk_qsgd", 8), ("topk_qsgd", 4)])
def test_bitmap_index_roundtrip(kind, bits):
    """K = 0.4: bitmap-indexed tensors decode to the same entries as the u16 index list."""
    numels = [8192 * 3 + 77, 3, 500, 40000]
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    auto = BucketPlan(numels, offs, 0.4, 0, o)
    lst = BucketPlan(numels, offs, 0.4, 0, o, index_mode="list")
    assert auto.tensor_bm0 == [0, -1, 771, 787] and auto.tensor_idx0 == [-1, 0, -1, -1]
    la, ll = Layout.build(kind, auto, bits), Layout.build(kind, lst, bits)
    assert la.nbytes < (0.8 if kind == "topk" else 0.6) * ll.nbytes
    g = torch.randn(o)
    levels = 127 if bits == 8 else 7
    pa = oracle.encode_topk(g.clone(), auto, la, levels, "max", 9)
    pl = oracle.encode_topk(g.clone(), lst, ll, levels, "max", 9)
    da = oracle.decode_sum(torch.stack([pa, pa]), auto, la, levels, 0.5)
    dl = oracle.decode_sum(torch.stack([pl, pl]), lst, ll, levels, 0.5)
    assert torch.equal(da, dl)


def test_method5_bitmap_beats_published_bytes():
    """LeNet at the report's K = 0.4 with 8-bit codes: reference-equivalent bytes (2 workers x
    push + pull = 4 x payload) below the published 1.312 MB (Report.zip: Comm Cost.png)."""
    flat = FlatModel(build_model("LeNet"), bucket_bytes=1 << 40)
    p = flat.buckets[0].plan
    plan = BucketPlan(p.numels, p.offsets, 0.4, 0, p.length)
    lay = Layout.build("topk_qsgd", plan, 8)
    assert 4 * lay.nbytes / 2 ** 20 < 1.312
    assert 4 * lay.nbytes / 2 ** 20 / 20 < 0.066  # Method 6: every 20 iterations


def test_codec_set_ratio_replans():
    from ewdml.compress.codecs import make_codec

    c = make_codec("topk_qsgd", ratio=0.01).bind([_plan([100000, 5000], 1.0)], "cpu")
    n1 = c.payload_bytes(0)
    c.set_ratio(0.25)
    assert c.plans[0].ks == [25000, 1250] and c.payload_bytes(0) > 8 * n1
    c.set_ratio(0.01)
    assert c.payload_bytes(0) == n1 and c.plans[0].ks == [1000, 50]


def test_ef21_estimate_tracks_the_gradient():
    """EF21: h accumulates what was sent; with a constant gradient the estimate converges to it
    (the difference g - h shrinks every step), so nothing is ever sent in bursts."""
    plan = _plan([4000], 0.05)
    lay = Layout.build("topk", plan, 8)
    g = torch.randn(plan.length)
    h = torch.zeros(plan.length)
    G = torch.zeros(plan.length)
    errs = []
    for step in range(25):
        pay = oracle.encode_topk(g.clone(), plan, lay, 127, "max", step, residual=h, ef21=True)
        G += oracle.decode_sum(pay[None], plan, lay, 127, 1.0)
        errs.append(float((g[:4000] - G[:4000]).norm()))
    assert torch.equal(G, h)  # world of one: the global estimate is the local one
    assert errs[-1] < 0.3 * errs[0] and all(b <= a + 1e-6 for a, b in zip(errs, errs[1:]))


def test_plan_candidate_capacity_and_blocks():
    """Predictive top-k encode tables (compress/plan.py): a tensor keeps at most 8 k + 4096
    candidates (capped at numel), its candidate list starts after the previous tensor's, and its
    candidate passes get one block per 8192 entries of capacity."""
    import torch

    from ewdml.compress.plan import CAND_K_MULT, CAND_SLACK, CHUNK, BucketPlan

    numels = [20, 500, 2359296, 100003]
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    plan = BucketPlan(numels, offs, 0.01, 0, o)
    for n, k, cap in zip(plan.numels, plan.ks, plan.tensor_cap):
        assert cap == min(n, CAND_K_MULT * k + CAND_SLACK)
    assert plan.tensor_cap0 == [0, 20, 520, 520 + plan.tensor_cap[2]]
    assert plan.total_cap == sum(plan.tensor_cap)
    assert plan.tensor_cblocks == [max(1, -(-c // CHUNK)) for c in plan.tensor_cap]
    tt = plan.tensor_table("cpu")
    assert tt[:, 9].tolist() == plan.tensor_cap0 and tt[:, 10].tolist() == plan.tensor_cap
    cb = plan.cblock_table("cpu")
    assert cb.shape == (plan.num_cblocks, 2)
    for t, nb in enumerate(plan.tensor_cblocks):
        rows = cb[cb[:, 0] == t]
        assert rows[:, 1].tolist() == list(range(nb))


# ---- dense QSGD: the properties tests/kernels/test_qsgd_codec_hip.py leans on -------------------
@pytest.mark.parametrize("bits,levels", [(8, 127), (4, 7)])
@pytest.mark.parametrize("norm", ["max", "l2"])
def test_qsgd_error_feedback_conserves_the_gradient(norm, bits, levels):
    """sent + new residual == g + old residual: the new residual is the one fp32 rounding of
    ``e - sent``, so the identity holds to half an ulp of it, and exactly wherever that
    subtraction is exact."""
    from tests import qsgd_sim as sim

    plan = sim.make_plan([8192 + 13, 10, 5000, 1])
    lay = Layout.build("qsgd", plan, bits)
    g, r = sim.bucket(plan, 1), sim.bucket(plan, 2)
    e = g + r
    pay = oracle.encode_qsgd(g.clone(), plan, lay, levels, norm, rng.stream_key(3, 1, 0), r)
    sent = oracle.decode_sum(pay[None], plan, lay, levels, 1.0)
    for off, n in zip(plan.offsets, plan.numels):
        s, rn, x = (t[off:off + n].double() for t in (sent, r, e))
        assert bool(((s + rn - x).abs() <= 2.0 ** -24 * rn.abs()).all())
        assert int((s + rn == x).sum()) > n // 2  # Sterbenz: exact for every code but the smallest
        assert float(rn.abs().max()) <= float(x.abs().max() if norm == "max" else x.norm()) / levels


@pytest.mark.parametrize("norm,exps", [("max", (-70, -40, 40, 70)), ("l2", (-40, 40))])
def test_quantize_is_invariant_to_powers_of_two(norm, exps):
    """A gradient times 2^e has the codes of the gradient and 2^e times its scale, bit for bit."""
    n = 5000
    x = torch.randn(n, generator=torch.Generator().manual_seed(4)) * 0.1
    gidx, key = 77 + torch.arange(n), rng.stream_key(3, 2, 1)
    scale = oracle._scale_of(x, norm)
    for levels in (127, 7):
        q = oracle.quantize(x, scale, levels, gidx, key)
        assert int(q.abs().max()) == levels or norm == "l2"
        for e in exps:
            f = 2.0 ** e
            assert oracle._scale_of(x * f, norm) == float(np.float32(scale) * np.float32(f))
            assert torch.equal(oracle.quantize(x * f, oracle._scale_of(x * f, norm), levels, gidx,
                                               key), q)
            assert oracle.dequant_step(levels, scale * f) == oracle.dequant_step(levels, scale) * f


@pytest.mark.parametrize("bits,levels", [(8, 127), (4, 7)])
def test_qsgd_l2_unbiased(bits, levels):
    """The mean over K = 64 keys of the decoded L2-norm payload, every element, within 6 standard
    deviations' bound of the gradient (tests/qsgd_sim.py worst_z; the keys are counter-based, so
    the figure is deterministic: 3.6 at worst).  The kernels are held to the same 6."""
    from tests import qsgd_sim as sim

    plan = sim.make_plan(sim.UNBIASED)
    lay = Layout.build("qsgd", plan, bits)
    g = sim.bucket(plan, sim.UNBIASED_SEED)
    acc = torch.zeros(plan.length, dtype=torch.float64)
    for key in sim.UNBIASED_KEYS:
        pay = oracle.encode_qsgd(g.clone(), plan, lay, levels, "l2", key)
        acc += oracle.decode_sum(pay[None], plan, lay, levels, 1.0).double()
    z = sim.worst_z(plan, g, acc / len(sim.UNBIASED_KEYS), levels)
    print(f"\nqsgd-l2-unbiased oracle bits={bits} worst_z={z:.3f}")
    assert 1.0 < z <= sim.UNBIASED_Z
