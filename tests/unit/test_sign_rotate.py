"""The Hadamard-rotated sign codec on the CPU (compress/oracle.py encode_sign / decode_sum with
``rot_key``): the transform pair, the quality it buys on heavy-tailed chunks, the residual, the
unchanged payload layout and the CLI / config / API plumbing."""
import numpy as np
import pytest
import torch

import ewdml
from ewdml.compress import Codec, oracle
from ewdml.compress.plan import CHUNK, BucketPlan, Layout

KEY = oracle.hsign_rot_key(0, 0)


def _plan(numels, bucket_offset=0):
    offs, o = [], 0
    for n in numels:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return BucketPlan(numels, offs, 1.0, bucket_offset, o)


def _grad(plan, seed=0):
    g = torch.zeros(plan.length)
    gen = torch.Generator().manual_seed(seed)
    for off, n in zip(plan.offsets, plan.numels):
        g[off:off + n] = torch.randn(n, generator=gen) * (0.1 + torch.rand(1, generator=gen))
    return g


def _roundtrip(e, rot_key):
    """(decoded, residual) of one full chunk ``e`` through encode + decode of a world of one."""
    plan = _plan([CHUNK])
    lay = Layout.build("sign", plan)
    resid = torch.zeros(plan.length)
    pay = oracle.encode_sign(e.clone(), plan, lay, resid, rot_key)
    return oracle.decode_sum(pay[None], plan, lay, 0, 1.0, rot_key), resid


def _rel_err(e, d):
    return float(((e - d).double() ** 2).sum() / (e.double() ** 2).sum())


def test_stage_order_is_a_permutation_of_the_index_bits():
    assert sorted(oracle.HSIGN_STAGE_BITS) == list(range(13)) and 1 << 13 == CHUNK
    assert oracle.HSIGN_INV == 1.0 / CHUNK


def test_fwht_is_the_hadamard_matrix():
    """Column k of H is (-1)^popcount(i & k): checked on unit vectors (exact in fp32)."""
    ks = [0, 1, 5, 1024, 4097, 8191]
    x = torch.zeros(len(ks), CHUNK)
    for r, k in enumerate(ks):
        x[r, k] = 1.0
    got = oracle.fwht(x).numpy()
    i = np.arange(CHUNK)
    for r, k in enumerate(ks):
        par = np.array([bin(v).count("1") & 1 for v in (i & k)])
        assert np.array_equal(got[r], np.where(par == 1, -1.0, 1.0).astype(np.float32))


def test_involution_exact_on_integers():
    gen = torch.Generator().manual_seed(1)
    x = torch.randint(-1024, 1025, (3, CHUNK), generator=gen).float()
    back = oracle.fwht(oracle.fwht(x)) * oracle.HSIGN_INV
    assert torch.equal(back, x)


def test_flip_is_an_involution_on_every_bit_pattern():
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(2, CHUNK, generator=gen)
    x[0, :4] = torch.tensor([0.0, -0.0, float("nan"), float("inf")])
    once = oracle.hsign_flip(x, KEY)
    twice = oracle.hsign_flip(once, KEY)
    assert torch.equal(twice.view(torch.int32), x.view(torch.int32))
    changed = once.view(torch.int32) != x.view(torch.int32)
    assert 0.4 < float(changed.float().mean()) < 0.6  # about half of the sign bits flip
    assert torch.equal(once.view(torch.int32) & 0x7FFFFFFF, x.view(torch.int32) & 0x7FFFFFFF)
    # chunk row c of a taller input takes the words of row c: row0 addresses them
    assert torch.equal(oracle.hsign_flip(x[1:], KEY, row0=1).view(torch.int32),
                       once[1:].view(torch.int32))
    assert oracle.hsign_rot_key(0, 0) != oracle.hsign_rot_key(0, 1) != oracle.hsign_rot_key(1, 1)


def test_flip_words_follow_the_written_rule():
    from ewdml.compress.rng import mix32_int

    x = torch.ones(2, CHUNK)
    got = oracle.hsign_flip(x, KEY) < 0
    for c, w, k in [(0, 0, 0), (0, 7, 31), (1, 0, 3), (1, 255, 17)]:
        word = mix32_int((c * 256 + w) ^ KEY)
        assert bool(got[c, 32 * w + k]) == bool((word >> k) & 1)


def test_zero_chunk():
    plan = _plan([CHUNK, 100])
    lay = Layout.build("sign", plan)
    resid = torch.zeros(plan.length)
    pay = oracle.encode_sign(torch.zeros(plan.length), plan, lay, resid, KEY)
    scales = pay.numpy()[lay.scales:lay.scales + 8].view(np.float32)
    assert (scales == 0).all() and not resid.any()
    assert not oracle.decode_sum(pay[None], plan, lay, 0, 1.0, KEY).any()


def test_quality_heavy_tail():
    e = torch.randn(CHUNK, generator=torch.Generator().manual_seed(0)) ** 3
    d_rot, _ = _roundtrip(e, KEY)
    d_raw, _ = _roundtrip(e, None)
    err_rot, err_raw = _rel_err(e, d_rot), _rel_err(e, d_raw)
    print(f"relative error: rotated {err_rot:.4f}, unrotated {err_raw:.4f}")
    assert err_rot <= 0.40  # theory: 1 - 2 / pi = 0.363
    assert err_rot < 0.5 * err_raw


def test_one_hot_reconstructs_exactly():
    e = torch.zeros(CHUNK)
    e[1234] = -3.5
    d, resid = _roundtrip(e, KEY)
    assert torch.equal(d, e) and not resid.any()


def test_residual_is_what_was_not_sent():
    """residual = e - decoded to within 4 ulp of max|e| (both come out of the same inverse
    transform, one of e's rotation and one of the quantised row)."""
    plan = _plan([8192 * 2 + 5, 7, 700])
    lay = Layout.build("sign", plan)
    g = _grad(plan, seed=3)
    r0 = _grad(plan, seed=4) * 0.3
    resid = r0.clone()
    pay = oracle.encode_sign(g.clone(), plan, lay, resid, KEY)
    d = oracle.decode_sum(pay[None], plan, lay, 0, 1.0, KEY)
    keep = torch.ones(plan.length, dtype=torch.bool)
    for off, n in zip(plan.offsets, plan.numels):
        e = (g + r0)[off:off + n]
        tol = 4 * float(np.spacing(np.float32(e.abs().max())))
        dev = float((resid[off:off + n] - (e - d[off:off + n])).abs().max())
        print(f"tensor of {n}: max deviation {dev:.3e}, bound {tol:.3e}")
        assert dev <= tol
        keep[off:off + n] = False
    assert torch.equal(resid[keep], r0[keep])  # the gaps between the tensors are not touched
    assert not d[keep].any()


def test_decode_is_linear_across_ranks():
    """N ranks' payloads summed in the rotated domain, one inverse transform: equals the oracle's
    own definition written out per rank."""
    plan = _plan([8192 + 77, 33], bucket_offset=64)
    lay = Layout.build("sign", plan)
    N = 3
    pays = torch.stack([oracle.encode_sign(_grad(plan, seed=10 + r) * (10.0 ** r), plan, lay,
                                           None, KEY) for r in range(N)])
    got = oracle.decode_sum(pays, plan, lay, 0, 1.0 / N, KEY)
    a = torch.zeros(plan.num_chunks, CHUNK)
    for r in range(N):
        a = a + oracle._sign_rows(pays[r], plan, lay)
    want = oracle._sign_scatter(oracle.hsign_unrotate(a, KEY), plan) * torch.tensor(1.0 / N)
    assert torch.equal(got, want)
    mean = sum(_grad(plan, seed=10 + r) * (10.0 ** r) for r in range(N)) / N
    assert _rel_err(mean, got) < 0.45


def test_layout_is_the_sign_layout():
    plan = _plan([8192 * 3 + 5, 7, 64, 100003])
    plain = Codec("sign").bind([plan], "cpu")
    rot = Codec("sign", rotate="hadamard").bind([plan], "cpu")
    a, b = plain.layouts[0], rot.layouts[0]
    assert (a.kind, a.nbytes, a.scales, a.codes) == (b.kind, b.nbytes, b.scales, b.codes)
    assert rot.payload_bytes(0) == plain.payload_bytes(0)
    assert rot.describe() == "sign1b-h" and plain.describe() == "sign1b"
    assert rot.kind == "sign" and rot.rotate == "hadamard" and plain.rotate == "none"
    assert rot.rot_key(0) == oracle.hsign_rot_key(rot.seed, 0) and plain.rot_key(0) is None


def test_default_is_todays_codec_byte_for_byte():
    plan = _plan([500, 8192 + 10])
    lay = Layout.build("sign", plan)
    g = _grad(plan, seed=6)
    r1, r2 = torch.zeros(plan.length), torch.zeros(plan.length)
    assert torch.equal(oracle.encode_sign(g, plan, lay, r1, rot_key=None),
                       oracle.encode_sign(g, plan, lay, r2))
    assert torch.equal(r1, r2)
    c = Codec("sign").bind([plan], "cpu")
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8)
    c.encode(0, g, pay, step=0, rank=0)
    assert torch.equal(pay, oracle.encode_sign(g, plan, lay))
    cfg = ewdml.parse_args(["--compress", "sign", "--device", "cpu"])
    assert cfg.sign_rotate == "none"


def test_codec_cpu_roundtrip():
    plan = _plan([500, 8192 + 10])
    c = Codec("sign", rotate="hadamard", seed=7).bind([plan, plan], "cpu")
    lay = c.layouts[1]
    g = _grad(plan, seed=4)
    pay = torch.zeros(lay.nbytes, dtype=torch.uint8)
    resid, ref = torch.zeros(plan.length), torch.zeros(plan.length)
    c.encode(1, g, pay, step=3, rank=1, resid=resid)
    key = oracle.hsign_rot_key(7, 1)  # the bucket's key: no step, no rank
    assert torch.equal(pay, oracle.encode_sign(g, plan, lay, ref, key)) and torch.equal(resid, ref)
    assert not torch.equal(pay, oracle.encode_sign(g, plan, lay))
    out = torch.zeros(plan.length)
    c.decode(1, pay[None], out, 0.5)
    assert torch.equal(out, oracle.decode_sum(pay[None], plan, lay, 0, 0.5, key))
    with pytest.raises(ValueError, match="not rotated"):
        c.encode_momentum(1, g, pay, resid, g, 0.9)
    with pytest.raises(ValueError, match="not rotated"):
        c.bind_twostage([], "cpu")
    with pytest.raises(ValueError, match="sign codec"):
        Codec("topk", rotate="hadamard")
    with pytest.raises(ValueError, match="rotation"):
        Codec("sign", rotate="fourier")
    with pytest.raises(ValueError, match="sign codec"):
        oracle.decode_sum(pay[None], plan, Layout.build("qsgd", plan, 8), 127, 1.0, key)


def test_flags_and_refusals():
    base = ["--compress", "sign", "--sign-rotate", "hadamard", "--device", "cpu"]
    cfg = ewdml.parse_args(base)
    assert cfg.sign_rotate == "hadamard" and cfg.error_feedback is True
    with pytest.raises(ValueError, match="needs --compress sign"):
        ewdml.parse_args(["--compress", "topk_qsgd", "--sign-rotate", "hadamard", "--device", "cpu"])
    with pytest.raises(ValueError, match="twostage.*transform pair"):
        ewdml.parse_args(base + ["--topology", "twostage"])
    for opt in ("onebit_adam", "onebit_lamb"):
        with pytest.raises(ValueError, match="fused decode is not rotated"):
            ewdml.parse_args(base + ["--optimizer", opt, "--onebit-warmup-steps", "2"])
    # everything --compress sign refuses stays refused
    for bad in (["--topology", "ps"], ["--topology", "sharded"], ["--sync-every", "5"]):
        with pytest.raises(ValueError, match="sign"):
            ewdml.parse_args(base + bad)
    with pytest.raises(SystemExit):
        ewdml.parse_args(["--compress", "sign", "--sign-rotate", "fourier"])


def test_horovod_compression_and_engine_refusal():
    from ewdml.models import build_model
    from ewdml.optim import make_optimizer
    from ewdml.parallel.comm import Comm
    from ewdml.parallel.engine import GradientExchange
    from ewdml.parallel.flat import FlatModel
    from ewdml.parallel.horovod import Compression

    c = Compression.sign(rotate="hadamard")
    assert isinstance(c, Codec) and c.kind == "sign" and c.rotate == "hadamard"
    assert Compression.sign().rotate == "none"
    flat = FlatModel(build_model("LeNet"), bucket_bytes=16 << 20)
    opt = make_optimizer("sgd", flat, lr=0.01, momentum=0.9)
    ex = GradientExchange(flat, Comm(), c, opt, overlap=False, error_feedback=True)
    assert ex.ef_mode == "plain" and ex.resid is not None
    ex.close()
