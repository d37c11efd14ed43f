"""The SGD / Adam reference of the kernel tests (``tests/optim_ref.py``) against third parties:
``torch.optim`` in float64, the torch oracle run on float64 tensors, and ``FlatSGD`` / ``FlatAdam``
on a CPU ``FlatModel``.  The float64 comparisons agree to 1e-13 absolute (a few 1e-16 measured:
the same operations in another association)."""
import pytest
import torch

from ewdml.compress import oracle
from ewdml.optim import FlatAdam, FlatSGD
from tests import optim_ref as R
from tests.layerwise_ref import make_flat, make_grad

N = 3076
STEPS = 4
TOL64 = 1e-13
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)
SGD_CASES = {"plain": dict(lr=0.1),
             "momentum_dampening_wd": dict(lr=0.1, momentum=0.9, dampening=0.1, weight_decay=1e-3),
             "nesterov_wd": dict(lr=0.05, momentum=0.8, weight_decay=1e-3, nesterov=True)}


def _data(seed, pscale=1.0):
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(N, generator=gen) * pscale
    gs = [torch.randn(N, generator=gen) * (0.1 + float(torch.rand(1, generator=gen)))
          for _ in range(STEPS)]
    return p0, gs


@pytest.mark.parametrize("case", list(SGD_CASES))
def test_sgd64_equals_torch_optim_in_float64(case):
    hp = SGD_CASES[case]
    p0, gs = _data(1)
    p, buf = p0.double(), torch.zeros(N, dtype=torch.float64)
    q = torch.nn.Parameter(p0.double())
    opt = torch.optim.SGD([q], foreach=False, **hp)
    for s, g in enumerate(gs):
        R.sgd64(p, buf, g, first=s == 0, round_hp=False, **hp)
        q.grad = g.double()
        opt.step()
    e = R.err(q.detach(), p)
    print(f"sgd {case}: |ref64 - torch.optim| max {e:.2e}")
    assert e <= TOL64 and not torch.equal(p, p0.double())
    if hp.get("momentum"):
        assert R.err(opt.state[q]["momentum_buffer"], buf) <= TOL64


@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam64_equals_torch_optim_in_float64_at_eps_zero(amsgrad):
    """With eps = 0 ``sqrt(v) + eps`` and torch's ``sqrt(v) / sqrt(bc2) + eps`` are the same rule."""
    hp = dict(ADAM, eps=0.0)
    p0, gs = _data(2, 1e-3)
    p, m, v, vm = [p0.double()] + [torch.zeros(N, dtype=torch.float64) for _ in range(3)]
    q = torch.nn.Parameter(p0.double())
    opt = torch.optim.Adam([q], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=0.0,
                           weight_decay=hp["weight_decay"], amsgrad=amsgrad, foreach=False)
    for s, g in enumerate(gs):
        if amsgrad and s >= 2:
            g = g * 0.01  # v falls below its running maximum from here on
        R.adam64(p, m, v, vm, g, s + 1, amsgrad=amsgrad, round_hp=False, **hp)
        q.grad = g.double()
        opt.step()
    st = opt.state[q]
    errs = {"p": R.err(q.detach(), p), "exp_avg": R.err(st["exp_avg"], m),
            "exp_avg_sq": R.err(st["exp_avg_sq"], v)}
    if amsgrad:
        errs["max_exp_avg_sq"] = R.err(st["max_exp_avg_sq"], vm)
        assert float((vm > v).float().mean()) > 0.9
    print(f"adam amsgrad={amsgrad}: |ref64 - torch.optim| max {errs}")
    assert max(errs.values()) <= TOL64


@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam64_equals_the_oracle_on_float64_tensors(amsgrad):
    """eps > 0: torch.optim's form legitimately differs (1.6e-6 on these inputs), the project's
    own reference form, run in float64, does not."""
    p0, gs = _data(3, 1e-3)
    p, m, v, vm = [p0.double()] + [torch.zeros(N, dtype=torch.float64) for _ in range(3)]
    po, mo, vo, vmo = (x.clone() for x in (p, m, v, vm))
    for s, g in enumerate(gs):
        R.adam64(p, m, v, vm, g, s + 1, amsgrad=amsgrad, round_hp=False, **ADAM)
        oracle.adam_apply(po, mo, vo, vmo, g.double(), ADAM["lr"], ADAM["beta1"], ADAM["beta2"],
                          ADAM["eps"], ADAM["weight_decay"], s + 1, amsgrad)
    errs = [R.err(a, b) for a, b in ((po, p), (mo, m), (vo, v), (vmo, vm))]
    print(f"adam amsgrad={amsgrad}: |ref64 - oracle(float64)| max {errs}")
    assert max(errs) <= TOL64 and not torch.equal(p, p0.double())


def _sgd_both(hp, p0, gs, grad_scale=1.0):
    p64, b64 = p0.double(), torch.zeros(N, dtype=torch.float64)
    p32, b32 = p0.clone(), torch.zeros(N)
    for s, g in enumerate(gs):
        R.sgd64(p64, b64, g, first=s == 0, grad_scale=grad_scale, **hp)
        R.sgd32(p32, b32, g, first=s == 0, grad_scale=grad_scale, **hp)
    return {"p": (p32, p64), "mom": (b32, b64)}


def _adam_both(amsgrad, p0, gs, grad_scale=1.0):
    s64 = [p0.double()] + [torch.zeros(N, dtype=torch.float64) for _ in range(3)]
    s32 = [p0.clone()] + [torch.zeros(N) for _ in range(3)]
    for s, g in enumerate(gs):
        R.adam64(*s64, g, s + 1, amsgrad=amsgrad, grad_scale=grad_scale, **ADAM)
        step = R.lr_step64(ADAM["lr"], ADAM["beta1"], ADAM["beta2"], s + 1)
        R.adam32(*s32, g, step, amsgrad=amsgrad, grad_scale=grad_scale,
                 **{k: v for k, v in ADAM.items() if k != "lr"})
    names = ["p", "exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if amsgrad else [])
    return {k: (a, b) for k, a, b in zip(names, s32, s64)}


def _pin(tag, pairs):
    """ref32 within the kernel tests' bound of ref64 (by construction), and that bound's own
    baseline within what fp32 allows: per step at most 8 separately rounded operations per
    element, each off by half an ulp (2^-24 relative) of a value no larger than twice the
    tensor's largest (the state plus its increment)."""
    for name, (x32, x64) in pairs.items():
        e, _ = R.check(name, x32, x32, x64, tag)
        assert e <= 16 * STEPS * 2.0 ** -24 * float(x64.abs().max()), (tag, name, e)
        assert e > 0.0 or name == "mom"  # fp32 and float64 differ, or the state was never used


@pytest.mark.parametrize("case", list(SGD_CASES))
def test_sgd32_follows_sgd64(case):
    p0, gs = _data(4)
    _pin(f"sgd {case} ", _sgd_both(SGD_CASES[case], p0, gs, 1.0 / 3.0))


@pytest.mark.parametrize("amsgrad", [False, True])
def test_adam32_follows_adam64(amsgrad):
    p0, gs = _data(5, 1e-3)  # |p0| ~ lr: the bound resolves the update
    _pin(f"adam amsgrad={amsgrad} ", _adam_both(amsgrad, p0, gs, 1.0 / 3.0))


def test_double_betas_in_the_bias_correction_would_be_seen():
    """The fault the bound exists for: bias-correcting with the double betas (6.7e-6 relative in
    ``lr_step``) is outside the limit at |p0| ~ lr."""
    p0, gs = _data(5, 1e-3)
    want = _adam_both(False, p0, gs)["p"]
    s32 = [p0.clone()] + [torch.zeros(N) for _ in range(3)]
    for s, g in enumerate(gs):
        step = R.lr_step64(ADAM["lr"], ADAM["beta1"], ADAM["beta2"], s + 1, round_hp=False)
        R.adam32(*s32, g, step, **{k: v for k, v in ADAM.items() if k != "lr"})
    e, lim = R.err(s32[0], want[1]), R.limit(*want)
    print(f"double betas: err {e:.3e} limit {lim:.3e}")
    assert e > lim


@pytest.mark.parametrize("case", list(SGD_CASES))
def test_flat_sgd_on_the_cpu_follows_sgd64(case):
    hp = SGD_CASES[case]
    flat = make_flat()
    p0 = flat.data.detach().clone()
    n = flat.numel
    opt = FlatSGD(flat, **hp)
    p64, b64 = p0.double(), torch.zeros(n, dtype=torch.float64)
    p32, b32 = p0.clone(), torch.zeros(n)
    for s in range(STEPS):
        g = make_grad(flat, s)
        opt.step(grad=g, grad_scale=0.5)
        R.sgd64(p64, b64, g, first=s == 0, grad_scale=0.5, **hp)
        R.sgd32(p32, b32, g, first=s == 0, grad_scale=0.5, **hp)
    assert opt.steps == STEPS
    R.check("p", flat.data.detach(), p32, p64, f"FlatSGD {case} ")
    R.check("mom", opt.mom, b32, b64, f"FlatSGD {case} ")


@pytest.mark.parametrize("amsgrad", [False, True])
def test_flat_adam_on_the_cpu_follows_adam64(amsgrad):
    flat = make_flat()
    p0 = flat.data.detach().clone()
    n = flat.numel
    opt = FlatAdam(flat, lr=ADAM["lr"], betas=(ADAM["beta1"], ADAM["beta2"]), eps=ADAM["eps"],
                   weight_decay=ADAM["weight_decay"], amsgrad=amsgrad)
    s64 = [p0.double()] + [torch.zeros(n, dtype=torch.float64) for _ in range(3)]
    s32 = [p0.clone()] + [torch.zeros(n) for _ in range(3)]
    for s in range(STEPS):
        g = make_grad(flat, s)
        opt.step(grad=g, grad_scale=0.5)
        R.adam64(*s64, g, s + 1, amsgrad=amsgrad, grad_scale=0.5, **ADAM)
        R.adam32(*s32, g, R.lr_step64(ADAM["lr"], ADAM["beta1"], ADAM["beta2"], s + 1),
                 amsgrad=amsgrad, grad_scale=0.5,
                 **{k: v for k, v in ADAM.items() if k != "lr"})
    got = [flat.data.detach(), opt.exp_avg, opt.exp_avg_sq] + \
        ([opt.max_exp_avg_sq] if amsgrad else [])
    for name, x, x32, x64 in zip(("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"), got, s32, s64):
        R.check(name, x, x32, x64, f"FlatAdam amsgrad={amsgrad} ")
