"""The threshold-search sparsifier on the CPU (compress/oracle.py encode_thresh): the oracle against
the independent numpy simulation (tests/thresh_sim.py) byte for byte, the payload's invariants,
the exact error-feedback identity, the layout's size, how full the slots get, and the codec
object, the Horovod-style constructor and the command line."""
import numpy as np
import pytest
import torch

import ewdml
from ewdml.compress import oracle
from ewdml.compress.codecs import Codec
from ewdml.compress.plan import BucketPlan, Layout
from ewdml.parallel.engine import plan_graph_mode
from tests import thresh_sim as sim


def _plan(numels=sim.NUMELS, ratio=sim.RATIO, dense_below=sim.DENSE_BELOW,
          bucket_offset=sim.BUCKET_OFFSET):
    offs, length = sim.offsets(numels)
    return BucketPlan(list(numels), offs, ratio, bucket_offset, length, dense_below)


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def shared():
    """The shared bucket encoded once by the oracle and once by the simulation, without a
    residual and over two steps with one."""
    plan = _plan()
    lay = Layout.build("thresh", plan)
    offs, length = sim.offsets()
    out = {"plan": plan, "lay": lay, "offs": offs, "length": length}
    g0, g1 = sim.bucket(0), sim.bucket(2)
    out["g"] = (g0, g1)
    out["o_plain"] = oracle.encode_thresh(torch.from_numpy(g0), plan, lay)
    out["s_plain"] = sim.encode(g0, sim.NUMELS, offs)
    r_o = torch.from_numpy(sim.bucket(1) * np.float32(0.25))
    r_o[torch.isnan(r_o) | torch.isinf(r_o)] = 0.5
    r_s = r_o.numpy().copy()
    out["r0"] = r_s.copy()
    out["o_ef"], out["s_ef"] = [], []
    for g in (g0, g1):
        pay = oracle.encode_thresh(torch.from_numpy(g), plan, lay, r_o)
        out["o_ef"].append((pay, r_o.clone()))
        s_pay, js, r_s = sim.encode(g, sim.NUMELS, offs, r_s)
        out["s_ef"].append((s_pay, js, r_s))
    return out


def test_plan_tables_against_sim(shared):
    plan = shared["plan"]
    cap, slot0, S = plan.thresh_slots()
    s_cap, s_slot0 = sim.caps(sim.NUMELS, shared["offs"])
    assert cap == s_cap and slot0 == s_slot0 and S == sum(s_cap)
    # the short last chunk keeps one slot, the tensors of up to 64 elements go whole
    assert cap[:4] == [82, 82, 82, 1] and cap[4] == 1 and cap[5] == 64 and cap[6] == 3
    assert plan.thresh_table("cpu").tolist() == [list(v) for v in zip(cap, slot0)]


def test_layout_size(shared):
    plan, lay = shared["plan"], shared["lay"]
    C = plan.num_chunks
    S = plan.thresh_slots()[2]
    a = lambda n: (n + 15) // 16 * 16
    assert (lay.counts, lay.idx, lay.codes) == (0, a(2 * C), a(a(2 * C) + 2 * S))
    assert lay.nbytes == a(lay.codes + 4 * S) and lay.bits == 32
    assert (lay.idx, lay.codes, lay.nbytes) == sim.layout(sim.NUMELS, shared["offs"])[:3]
    # 6 bytes per slot and 2 per chunk row, to within three alignment pads
    assert 0 <= lay.nbytes - (6 * S + 2 * C) < 48
    # a whole model at 1 %: the fp32 top-k codec's size to within the rounding of the capacities
    big = BucketPlan([512 * 512 * 9, 512, 4096 * 512], [0, 512 * 512 * 9, 512 * 512 * 9 + 512],
                     0.01)
    tk, th = Layout.build("topk", big).nbytes, Layout.build("thresh", big).nbytes
    assert abs(th - tk) / tk < 0.02


def test_threshold_rule_against_brute_force():
    """oracle.thresh_threshold (a sort) against trying every J (the simulation), on chunks with
    ties at the boundary, all-equal chunks, chunks that fit whole and non-finite values."""
    rs = np.random.RandomState(5)
    cases = [(rs.standard_normal(8192).astype(np.float32), 82),
             ((rs.standard_normal(8192) ** 3).astype(np.float32), 8),
             (np.full(300, 0.375, np.float32), 3), (np.zeros(64, np.float32), 64),
             (np.float32([1, 1, 1, 2, 2, 3]), 2), (np.float32([1, 1, 1, 2, 2, 3]), 3),
             (np.float32([5.0]), 1), (np.float32([np.nan, np.inf, 1, 1, -np.inf]), 2),
             (np.float32([3, 3, 3]), 1), (rs.standard_normal(5).astype(np.float32), 1)]
    for x, cap in cases:
        lev = oracle.thresh_level(torch.from_numpy(x))
        assert np.array_equal(lev.numpy(), sim.levels(x))
        J = oracle.thresh_threshold(lev, cap)
        assert J == sim.threshold(sim.levels(x), cap), (x[:6], cap)
        assert int((lev >= J).sum()) <= cap and (J == 0 or int((lev >= J - 1).sum()) > cap)
    assert oracle.thresh_threshold(oracle.thresh_level(torch.tensor([3.0, 3.0, 3.0])), 1) == \
        (0x4040 + 1)  # all tie: the threshold sits one above their level and nothing is sent
    assert int(oracle.thresh_level(torch.tensor([float("nan")]))) > \
        int(oracle.thresh_level(torch.tensor([float("inf")]))) == 0x7F80


def test_payload_bytewise_against_sim(shared):
    assert np.array_equal(shared["o_plain"].numpy(), shared["s_plain"][0])
    for (o_pay, o_res), (s_pay, _, s_res) in zip(shared["o_ef"], shared["s_ef"]):
        assert np.array_equal(o_pay.numpy(), s_pay)
        assert np.array_equal(_bits(o_res.numpy()), _bits(s_res))
    # the two steps differ, and the constant tensor (every level ties) is never sent
    assert not np.array_equal(shared["s_ef"][0][0], shared["s_ef"][1][0])


def test_payload_invariants(shared):
    plan, lay = shared["plan"], shared["lay"]
    cap, slot0, S = plan.thresh_slots()
    for pay in (shared["o_plain"], shared["o_ef"][0][0], shared["o_ef"][1][0]):
        counts = oracle._section(pay, lay.counts, plan.num_chunks, torch.int16).numpy() \
            .astype(np.int64) & 0xFFFF
        idx = oracle._section(pay, lay.idx, S, torch.int16).numpy().astype(np.int64) & 0xFFFF
        vals = oracle._section(pay, lay.codes, S, torch.float32).numpy()
        for c in range(plan.num_chunks):
            m = counts[c]
            assert m <= cap[c]
            own = idx[slot0[c]:slot0[c] + cap[c]]
            assert np.all(np.diff(own[:m]) > 0) and np.all(own[:m] < plan.chunk_len[c])
            assert not own[m:].any()
            assert not _bits(vals[slot0[c] + m:slot0[c] + cap[c]]).any()  # +0.0, not -0.0
        t0 = plan.tensor_chunk0
        assert counts[t0[sim.CONST_T]] == 0  # all tie
        assert counts[t0[sim.ZERO_T]] == 64 and counts[t0[sim.WHOLE_T]] == 40  # sent whole
        assert counts[t0[1]] == 1  # the one-element tensor
        sent = idx[slot0[t0[sim.NONFINITE_T]]:][:counts[t0[sim.NONFINITE_T]]].tolist()
        assert sim.NAN_AT in sent and sim.INF_AT in sent


def test_decode_against_sim(shared):
    plan, lay = shared["plan"], shared["lay"]
    pays = [shared["o_plain"], shared["o_ef"][0][0], shared["o_ef"][1][0]]
    for n in (1, 2, 3):
        recv = torch.stack(pays[:n])
        got = oracle.decode_sum(recv, plan, lay, 1, 1.0 / n).numpy()
        want = sim.decode_mean([p.numpy() for p in pays[:n]], sim.NUMELS, shared["offs"],
                               shared["length"], 1.0 / n)
        assert np.array_equal(_bits(got), _bits(want))


def test_decode_clamps_a_corrupt_row(shared):
    """A count of 0xFFFF reads the chunk's own slots and no further, and an index at or past the
    chunk's length is dropped."""
    plan, lay = shared["plan"], shared["lay"]
    cap, slot0, S = plan.thresh_slots()
    pay = shared["o_plain"].clone()
    counts = oracle._section(pay, lay.counts, plan.num_chunks, torch.int16)
    idx = oracle._section(pay, lay.idx, S, torch.int16)
    vals = oracle._section(pay, lay.codes, S, torch.float32)
    counts[:] = -1
    c = 3  # the five-element chunk with one slot
    idx[slot0[c]] = 5
    c = plan.tensor_chunk0[sim.CUBED_T] + 1  # 808 elements, 9 slots
    idx[slot0[c]:slot0[c] + 9] = torch.tensor([0, 807, 808, 8191, -1, 1, 2, 3, 4],
                                              dtype=torch.int16)
    vals[slot0[c]:slot0[c] + 9] = torch.arange(1.0, 10.0)
    got = oracle.decode_sum(pay[None], plan, lay, 1, 1.0).numpy()
    want = sim.decode(pay.numpy(), sim.NUMELS, shared["offs"], shared["length"])
    assert np.array_equal(_bits(got), _bits(want))
    s0 = plan.chunk_start[c]
    assert got[s0:s0 + 5].tolist() == [1.0, 6.0, 7.0, 8.0, 9.0] and got[s0 + 807] == 2.0
    assert not got[plan.chunk_start[3]:plan.chunk_start[3] + 5].any()


def test_error_feedback_identity(shared):
    """decode(encode) + residual == acc bit for bit on every tensor position: a value is either
    sent exactly (residual +0.0) or kept exactly (decoded +0.0)."""
    plan, lay = shared["plan"], shared["lay"]
    r_prev = shared["r0"]
    for g, (pay, res) in zip(shared["g"], shared["o_ef"]):
        with np.errstate(invalid="ignore"):
            acc = (g + r_prev).astype(np.float32)
        dec = oracle.decode_sum(pay[None], plan, lay, 1, 1.0).numpy()
        res = res.numpy()
        for o, n in zip(plan.offsets, plan.numels):
            a, d, r = acc[o:o + n], dec[o:o + n], res[o:o + n]
            sent = _bits(r) == 0
            assert np.array_equal(_bits(np.where(sent, d, r)), _bits(a + np.float32(0.0)))
            assert not _bits(d[~sent]).any()
        r_prev = res


def test_slots_fill():
    """How full the slots get: ties at the boundary level are left out, so a chunk sends fewer
    than cap entries.  Over 200 chunks of 8192 fixed-seed values (N(0, 1) and its cube,
    alternating) the mean count / cap is at least 0.95 and the minimum at least 0.70, at the
    capacities of ratios 1 %, 0.25 % and 0.1 %."""
    rs = np.random.RandomState(2024)
    chunks = []
    for c in range(200):
        x = rs.standard_normal(8192)
        chunks.append((x ** 3 if c % 2 else x).astype(np.float32))
    for cap in (82, 21, 8):
        fill = []
        for x in chunks:
            lev = oracle.thresh_level(torch.from_numpy(x))
            fill.append(int((lev >= oracle.thresh_threshold(lev, cap)).sum()) / cap)
        print(f"cap {cap}: mean fill {np.mean(fill):.3f}, min {np.min(fill):.3f}")
        assert np.mean(fill) >= 0.95 and np.min(fill) >= 0.70


def test_codec_object(shared):
    plan, lay = shared["plan"], shared["lay"]
    assert Codec("thresh", ratio=0.01).describe() == "thresh-k0.01"
    assert Codec("thresh", ratio=0.25).describe() == "thresh-k0.25"
    c = Codec("thresh", ratio=sim.RATIO, dense_below=sim.DENSE_BELOW).bind(
        [BucketPlan(list(sim.NUMELS), shared["offs"], 1.0, sim.BUCKET_OFFSET, shared["length"])],
        "cpu")
    assert c.layouts[0] == lay and c.payload_bytes(0) == lay.nbytes  # rebound at its own ratio
    pay = torch.full((lay.nbytes + 32,), 0xFF, dtype=torch.uint8)
    c.encode(0, torch.from_numpy(shared["g"][0]), pay, 7, 1)
    assert torch.equal(pay[:lay.nbytes], shared["o_plain"])
    out = torch.zeros(plan.length)
    c.decode(0, pay[None, :lay.nbytes], out, 0.5)
    assert np.array_equal(_bits(out.numpy()), _bits(oracle.decode_sum(
        pay[None, :lay.nbytes], plan, lay, 1, 0.5).numpy()))
    with pytest.raises(ValueError, match="no encode-side apply"):
        c.encode(0, torch.zeros(plan.length), pay, 1, 0, apply={})
    # another density: fewer slots, the same chunk rows
    c.set_ratio(0.001)
    assert c.describe() == "thresh-k0.001" and c.payload_bytes(0) < lay.nbytes
    assert c.plans[0].num_chunks == plan.num_chunks
    # planned and predicted as the top-k payload it is
    got = plan_graph_mode(4, "rccl-stream", "thresh", 1 << 20, topk_ratio=0.01)
    assert got["mode"] == "full" and got["wire_bytes"] == int(3 * (1 << 20) * 0.01 * 6)
    tk = plan_graph_mode(1, "rccl-stream", "topk", 9_000_000, model="vgg11", topk_ratio=0.01)
    th = plan_graph_mode(1, "rccl-stream", "thresh", 9_000_000, model="vgg11", topk_ratio=0.01)
    assert th["mode"] == "full" and th.get("predicted_ms") == tk.get("predicted_ms")


def test_horovod_compression():
    from ewdml.parallel.horovod import Compression

    assert Compression.thresh().describe() == "thresh-k0.01"
    assert Compression.thresh(ratio=0.05).describe() == "thresh-k0.05"


def _resolve(*flags):
    return ewdml.parse_args(["--compress", "thresh", *flags]).resolved()


def test_cli():
    c = _resolve()
    assert c.error_feedback is True and c.topk_warmup == "" and c.lr_warmup_epochs == 0
    assert _resolve("--no-error-feedback").error_feedback is False
    # what the benchmark always passes is accepted
    c = _resolve("--qsgd-bits", "4", "--qsgd-levels", "7", "--error-feedback", "--ef-warmup",
                 "none", "--topk-ratio", "0.05", "--topk-dense-below", "64")
    assert c.topk_ratio == 0.05 and c.topk_dense_below == 64
    for opt in ("adam", "lars", "lamb", "lion"):
        assert _resolve("--optimizer", opt).optimizer == opt
    assert _resolve("--clip-grad-norm", "1.0").clip_grad_norm == 1.0
    assert _resolve("--hip-graph", "full").hip_graph == "full"


@pytest.mark.parametrize("flags,reason", [
    (["--topology", "ps"], "--topology ps"),
    (["--topology", "sharded"], "--topology sharded"),
    (["--topology", "twostage"], "--topology twostage"),
    (["--sync-every", "4"], "--sync-every"),
    (["--select-best"], "--select-best"),
    (["--ef-mode", "plain"], "--ef-mode plain"),
    (["--ef-mode", "ef21"], "--ef-mode ef21"),
    (["--optimizer", "onebit_adam", "--onebit-warmup-steps", "2"], "onebit_adam"),
    (["--optimizer", "onebit_lamb", "--onebit-warmup-steps", "2"], "onebit_lamb"),
])
def test_cli_refusals(flags, reason):
    with pytest.raises(ValueError, match="--compress thresh .*" + reason):
        _resolve(*flags)


def test_cli_refuses_the_pull_and_the_rotation():
    from ewdml.config import Config

    with pytest.raises(SystemExit):  # the pull codecs' choices stay as they were
        ewdml.parse_args(["--topology", "ps", "--pull-compress", "thresh"])
    with pytest.raises(ValueError, match="--pull-compress thresh"):
        Config(topology="ps", compress="qsgd", pull_compress="thresh").resolved()
    with pytest.raises(ValueError, match="--compress thresh has no parameter-server form"):
        Config(compress="thresh", pull_compress="qsgd").resolved()
    with pytest.raises(ValueError, match="--sign-rotate hadamard rotates the sign codec"):
        _resolve("--sign-rotate", "hadamard")
