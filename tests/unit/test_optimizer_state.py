"""Every name ``make_optimizer`` accepts, held to the same checks on the CPU: the class it
returns, the ``kind`` and exact key set of its ``state_dict()`` (a checkpoint's format), a
save / load round trip that continues bitwise, and that keywords an optimizer does not take, or
that are ``None``, change nothing."""
import pytest
import torch

from ewdml import optim
from ewdml.optim import make_optimizer
from tests.layerwise_ref import make_flat, make_grad

# a matrix GaLore and APOLLO project at rank 16 (short side 32), a vector and a 4-d weight whose
# [8, 36] view they keep dense; the matrix fills the first bucket
SHAPES = [(32, 48), (20,), (8, 4, 3, 3)]
BUCKET_BYTES = 4 * 32 * 48

_ADAM = {"kind", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "steps", "lr"}
_LAMB = {"kind", "exp_avg", "exp_avg_sq", "steps", "ratio", "lr", "weight_decay"}
# name -> (class, state_dict()["kind"], the keys of state_dict())
TABLE = {
    "sgd": ("FlatSGD", "sgd", {"kind", "mom", "steps", "lr", "momentum", "dampening",
                               "weight_decay", "nesterov"}),
    "adam": ("FlatAdam", "adam", _ADAM),
    "amsgrad": ("FlatAdam", "adam", _ADAM),
    "onebit_adam": ("FlatOnebitAdam", "onebit_adam", _ADAM | {"freeze_step"}),
    "adam8bit": ("FlatAdam8bit", "adam8bit", {"kind", "code_m", "code_v", "absmax_m", "absmax_v",
                                              "steps", "lr"}),
    "lion": ("FlatLion", "lion", {"kind", "exp_avg", "steps", "lr"}),
    "lars": ("FlatLARS", "lars", {"kind", "mom", "steps", "ratio", "lr", "momentum", "dampening",
                                  "weight_decay", "nesterov", "eta"}),
    "lamb": ("FlatLAMB", "lamb", _LAMB),
    "onebit_lamb": ("FlatOnebitLamb", "onebit_lamb", _LAMB | {
        "freeze_step", "exp_avg_sq_fresh", "coeff_ema", "r_frozen", "last_factor", "coeff_beta",
        "factor_min", "factor_max", "factor_threshold"}),
    "muon": ("FlatMuon", "muon", {"kind", "mom", "steps", "lr", "momentum", "weight_decay",
                                  "nesterov", "ns_steps", "ns_dtype", "aux_ratio"}),
    "adafactor": ("FlatAdafactor", "adafactor", {"kind", "row", "col", "v", "m", "steps", "lr"}),
    "galore": ("FlatGalore", "galore", {"kind", "proj", "m_lr", "v_lr", "m", "v", "steps", "lr"}),
    "apollo": ("FlatApollo", "apollo", {"kind", "m_lr", "v_lr", "m", "v", "norms", "steps", "lr",
                                        "seed"}),
}
# the keywords every optimizer is offered (the trainer's), freeze_step past the steps taken here
COMMON = dict(lr=0.01, momentum=0.9, dampening=0.0, weight_decay=0.01, nesterov=False, eps=1e-8,
              freeze_step=5, eta=0.001, seed=3)
# the options that belong to one optimizer each, all unset
UNSET = dict.fromkeys(
    ("betas", "ns_steps", "ns_dtype", "aux_lr", "adafactor_beta1", "adafactor_clip",
     "adafactor_scale_parameter", "galore_rank", "galore_update_gap", "galore_scale",
     "apollo_rank", "apollo_update_gap", "apollo_scale", "apollo_scale_type"))
# what makes the low-rank pair project the matrix and refresh within three steps
OWN = {"galore": dict(galore_rank=16, galore_update_gap=2),
       "apollo": dict(apollo_rank=16, apollo_update_gap=2),
       "adafactor": dict(adafactor_beta1=0.9)}


def _flat():
    flat = make_flat(shapes=SHAPES, seed=2, bucket_bytes=BUCKET_BYTES)
    assert len(flat.buckets) >= 2
    return flat


def _fields(opt):
    """The optimizer's own values: every plain attribute, and every tensor it holds."""
    plain, tensors = {}, {}
    for k, v in vars(opt).items():
        if torch.is_tensor(v):
            tensors[k] = v
        elif v is None or isinstance(v, (bool, int, float, str, tuple, list)):
            plain[k] = v
    return plain, tensors


@pytest.mark.parametrize("name", sorted(TABLE))
def test_class_kind_and_keys(name):
    cls, kind, keys = TABLE[name]
    opt = make_optimizer(name.upper(), _flat(), **COMMON)
    assert type(opt) is getattr(optim.flat, cls)
    sd = opt.state_dict()
    assert sd["kind"] == kind and set(sd) == keys
    if "max_exp_avg_sq" in sd:
        assert (sd["max_exp_avg_sq"] is not None) == (name == "amsgrad")


@pytest.mark.parametrize("name", sorted(TABLE))
def test_a_checkpoint_continues_bitwise(name):
    kw = dict(COMMON, **OWN.get(name, {}))
    flats = [_flat(), _flat()]
    first = make_optimizer(name, flats[0], **kw)
    for s in range(2):
        first.step(grad=make_grad(flats[0], s))
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in first.state_dict().items()}
    rest = make_optimizer(name, flats[1], **dict(kw, lr=0.5))
    flats[1].data.copy_(flats[0].data)
    rest.load_state_dict(sd)
    assert rest.steps == first.steps == 2 and rest.lr == first.lr == 0.01
    g = make_grad(flats[0], 2)
    first.step(grad=g)
    rest.step(grad=g)
    assert torch.equal(flats[1].data.view(torch.int32), flats[0].data.view(torch.int32))
    a, b = first.state_dict(), rest.state_dict()
    assert set(a) == set(b)
    for k, v in a.items():
        if torch.is_tensor(v):
            assert v.dtype == b[k].dtype and torch.equal(v, b[k]), k
            assert bool(v.ne(0).any()), f"{k} was never written"
        else:
            assert v == b[k], k


@pytest.mark.parametrize("name", sorted(TABLE))
def test_foreign_and_unset_keywords_change_nothing(name):
    bare = make_optimizer(name, _flat(), **COMMON)
    full = make_optimizer(name, _flat(), **COMMON, **UNSET)
    (plain_a, tens_a), (plain_b, tens_b) = _fields(bare), _fields(full)
    assert plain_a == plain_b
    assert set(tens_a) == set(tens_b)
    for k, v in tens_a.items():
        assert torch.equal(v, tens_b[k]), k
    sa, sb = bare.state_dict(), full.state_dict()
    assert {k: v for k, v in sa.items() if not torch.is_tensor(v)} == \
        {k: v for k, v in sb.items() if not torch.is_tensor(v)}


def test_names_it_refuses():
    with pytest.raises(ValueError, match="unknown optimizer"):
        make_optimizer("adagrad", _flat(), **COMMON)
    with pytest.raises(ValueError, match="8-bit Adam has no AMSGrad"):
        make_optimizer("adam8bit", _flat(), amsgrad=True, **COMMON)
