"""No GPU: the restatements of tests/optim_ext_ref.py tied to torch and to hand-computed values, their fp32 floors measured again
(a recorded FLOOR entry must lie within [measured / 1.25, 2 x measured], as in tests/test_streaming_ref_cpu.py), and the host
logic of the clipping / EMA layer: the decay schedule, the argparse refusals, the checkpoint overlay, and that neither feature
shows in an optimizer's state_dict().  `pytest -s` prints the measured floors.

The tests of the first group (the two by-hand restatements, test_floors, the size check) call nothing of the product, as
tests/test_streaming_ref_cpu.py does not: they pin the reference the GPU tests lean on and pass with or without the feature.
Every other test here needs the new API and fails without it."""
import collections
import contextlib

import pytest
import torch

from tests import optim_ext_ref as X
from tests.util import rel_err


@contextlib.contextmanager
def one_thread():
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(old)


def put(d, k, v):
    d[k] = max(d.get(k, 0.0), v)


# ---- restatements ----------------------------------------------------------------------------------------------------
def test_clipped_sgd_step_by_hand():
    """one nesterov step with the clip factor written out"""
    p0, grads = X.step_inputs(7)
    cfg = (0.9, True, 1e-4)
    mx = X.clipping_max_norm(grads)
    r = X.sgd_ext_ref(p0, grads[:1], cfg, max_norm=mx)
    g = grads[0].double()
    norm = float(g.norm())
    assert abs(r["norms"][0] - norm) < 1e-14 * norm and abs(X.norm64(grads[0].numpy()) - norm) < 1e-14 * norm
    coef = mx / (norm + 1e-6)
    assert 0.49 < coef < 0.51 and X.coef64(norm, mx) == coef and X.coef64(norm, 1e9) == 1.0
    d = g * coef + X.f32(1e-4) * p0.double()
    assert rel_err(r["buf"], d) < 1e-15 and rel_err(r["p"], p0.double() - X.SGD_LR * (d + X.f32(0.9) * d)) < 1e-15
    # a bound far above the norm changes nothing
    a, b = X.sgd_ext_ref(p0, grads, cfg, max_norm=1e9), X.sgd_ext_ref(p0, grads, cfg)
    assert torch.equal(a["p"], b["p"]) and torch.equal(a["buf"], b["buf"])


def test_ema_recurrence_by_hand():
    p0, grads = X.step_inputs(5, 3)
    r = X.sgd_ext_ref(p0, grads, (0.0, False, 0.0), ema=(0.5, True))
    p, avg = p0.double(), p0.double()
    for t, g in enumerate(grads, 1):
        p = p - X.SGD_LR * g.double()
        w = X.f32(1 - min(0.5, (1 + t) / (10 + t)))
        avg = avg + w * (p - avg)
    assert rel_err(r["p"], p) < 1e-15 and rel_err(r["ema"], avg) < 1e-15
    assert X.ema_weight(0.5, 1, True) == X.f32(9 / 11) and X.ema_weight(0.5, 1, False) == 0.5


def test_floors():
    m = {}
    with one_thread():
        for n in X.STEP_N:
            p0, grads = X.step_inputs(n)
            mx = X.clipping_max_norm(grads)
            for cfg in X.SGD_CONFIGS:
                a, b = X.sgd_ext_ref(p0, grads, cfg, mx), X.sgd_ext_ref(p0, grads, cfg, mx, dtype=torch.float32)
                put(m, "clip_sgd.p", rel_err(b["p"], a["p"]))
                put(m, "clip_sgd.buf", rel_err(b["buf"], a["buf"]))
            for cfg in X.ADAM_CONFIGS:
                a, b = X.adam_ext_ref(p0, grads, cfg, mx), X.adam_ext_ref(p0, grads, cfg, mx, dtype=torch.float32)
                for k in "pmv":
                    put(m, "clip_adam." + k, rel_err(b[k], a[k]))
            for steps, warm in X.EMA_SERIES:
                p0, grads = X.step_inputs(n, steps)
                for cfg in X.SGD_CONFIGS:
                    a = X.sgd_ext_ref(p0, grads, cfg, ema=(X.EMA_DECAY, warm))
                    b = X.sgd_ext_ref(p0, grads, cfg, ema=(X.EMA_DECAY, warm), dtype=torch.float32)
                    put(m, "ema_sgd.ema", rel_err(b["ema"], a["ema"]))
                for cfg in X.ADAM_CONFIGS:
                    a = X.adam_ext_ref(p0, grads, cfg, ema=(X.EMA_DECAY, warm))
                    b = X.adam_ext_ref(p0, grads, cfg, ema=(X.EMA_DECAY, warm), dtype=torch.float32)
                    put(m, "ema_adam.ema", rel_err(b["ema"], a["ema"]))
        for family, index in X.BIG_CASES:              # clip and EMA together at the second-trip size
            a, b = X.big_case(family, index)[4], X.big_case(family, index, torch.float32)[4]
            for k in ("p", "buf", "ema") if family == "sgd" else ("p", "m", "v", "ema"):
                put(m, "big_%s.%s" % (family, k), rel_err(b[k], a[k]))
    for k, v in sorted(m.items()):
        print("floor %-16s measured %.3e  recorded %.3e" % (k, v, X.FLOOR.get(k, float("nan"))))
    assert sorted(m) == sorted(X.FLOOR)
    for k, v in m.items():
        assert X.FLOOR[k] / 2 <= v <= 1.25 * X.FLOOR[k], "%s: measured %.3e, recorded %.3e" % (k, v, X.FLOOR[k])


def test_kernel_sizes_reach_the_second_trip():
    """the last raw-kernel size: 2048 workgroups x 256 threads cover 2048 * 256 float4s in one trip; one more float4 and a tail"""
    n = X.KERNEL_N[-1]
    assert n // 4 == 2048 * 256 + 1 and n % 4 == 1 and n < 2 ** 26


# ---- the decay schedule ----------------------------------------------------------------------------------------------
def test_decay_schedule():
    from iswm_amd.optim import ema_decay_at
    assert ema_decay_at(0.999, 1) == 2 / 11
    assert ema_decay_at(0.5, 7) == 8 / 17 and ema_decay_at(0.5, 8) == 0.5 and ema_decay_at(0.5, 9) == 0.5      # reaches decay at t = 8
    assert ema_decay_at(0.999, 1, warmup=False) == 0.999
    seq = [ema_decay_at(0.9, t) for t in range(1, 200)]
    assert all(a <= b for a, b in zip(seq, seq[1:])) and seq[-1] == 0.9 and seq[78] < 0.9 and seq[79] == 0.9  # (1+t)/(10+t) = .9 at t = 80
    for t in range(1, 30):
        assert ema_decay_at(0.5, t) == X.decay_at(0.5, t, True) and ema_decay_at(0.5, t, False) == X.decay_at(0.5, t, False)
    with pytest.raises(ValueError):
        ema_decay_at(0.9, 0)


# ---- argparse --------------------------------------------------------------------------------------------------------
CLIP_MSG, EMA_MSG, USE_MSG = "--clip_grad_norm must be", "--ema_decay must lie", "--use_ema evaluates"


@pytest.mark.parametrize("argv,message", [
    (["--clip_grad_norm", "-1"], CLIP_MSG), (["--clip_grad_norm", "nan"], CLIP_MSG), (["--clip_grad_norm", "inf"], CLIP_MSG),
    (["--ema_decay", "1"], EMA_MSG), (["--ema_decay", "-0.1"], EMA_MSG), (["--ema_decay", "nan"], EMA_MSG),
    (["--ema_decay", "1.5"], EMA_MSG),
    (["--use_ema"], USE_MSG), (["--use_ema", "--test_only"], USE_MSG), (["--use_ema", "--ckpt", "x.pth"], USE_MSG)])
def test_train_refuses_bad_values(argv, message, capsys):
    """the refusal is the new validation's own (argparse exits with 2 for an option it does not know, too)"""
    from iswm_amd import train
    with pytest.raises(SystemExit) as e:
        train.get_argparser().parse_args(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_train_accepts_and_defaults():
    from iswm_amd import predict, train
    o = train.get_argparser().parse_args([])
    assert o.clip_grad_norm == 0 and o.ema_decay == 0 and not o.ema_no_warmup and not o.use_ema
    o = train.get_argparser().parse_args(["--clip_grad_norm", "1.5", "--ema_decay", "0.999", "--ema_no_warmup"])
    assert o.clip_grad_norm == 1.5 and o.ema_decay == 0.999 and o.ema_no_warmup
    o = train.get_argparser().parse_args(["--test_only", "--use_ema", "--ckpt", "x.pth"])
    assert o.use_ema
    base = ["--input", "in", "--save_val_results_to", "out"]
    assert not predict.get_argparser().parse_args(base).use_ema
    assert predict.get_argparser().parse_args(base + ["--use_ema"]).use_ema


# ---- checkpoint overlay ----------------------------------------------------------------------------------------------
def test_ema_model_state_overlay():
    from iswm_amd.optim import ema_model_state
    live = collections.OrderedDict([("module.conv.weight", torch.ones(2, 3)), ("bn.weight", torch.ones(3)),
                                    ("bn.running_mean", torch.full((3,), 4.0))])
    ema = {"decay": 0.9, "warmup": True, "num_updates": 5,
           "params": {"conv.weight": torch.full((2, 3), 2.0), "bn.weight": torch.full((3,), 3.0)}}
    out = ema_model_state({"model_state": live, "ema_state": ema})
    assert list(out) == ["conv.weight", "bn.weight", "bn.running_mean"]
    assert torch.equal(out["conv.weight"], ema["params"]["conv.weight"]) and torch.equal(out["bn.weight"], ema["params"]["bn.weight"])
    assert torch.equal(out["bn.running_mean"], live["bn.running_mean"])            # buffers: the live statistics
    assert torch.equal(live["module.conv.weight"], torch.ones(2, 3))               # the checkpoint is not modified
    with pytest.raises(KeyError, match="ema_state"):
        ema_model_state({"model_state": live})
    ema["params"]["nope.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="nope.weight"):
        ema_model_state({"model_state": live, "ema_state": ema})


def test_load_model_use_ema_needs_ema_state(tmp_path):
    from iswm_amd import predict
    lin = torch.nn.Linear(2, 2)
    path = str(tmp_path / "plain.pth")
    torch.save({"model_state": lin.state_dict()}, path)
    with pytest.raises(KeyError, match="ema_state"):
        predict.load_model(torch.nn.Linear(2, 2), path, use_ema=True)
    with pytest.raises(FileNotFoundError):
        predict.load_model(torch.nn.Linear(2, 2), str(tmp_path / "none.pth"), use_ema=True)
    ema = {"decay": 0.5, "warmup": True, "num_updates": 1, "params": {"weight": torch.full((2, 2), 7.0), "bias": torch.zeros(2)}}
    torch.save({"model_state": lin.state_dict(), "ema_state": ema}, path)
    got = predict.load_model(torch.nn.Linear(2, 2), path, use_ema=True)
    assert torch.equal(got.weight.detach(), torch.full((2, 2), 7.0))
    assert torch.equal(predict.load_model(torch.nn.Linear(2, 2), path).weight.detach(), lin.weight.detach())


# ---- state_dict ------------------------------------------------------------------------------------------------------
def _params():
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(5, 3, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g))]


@pytest.mark.parametrize("family", ["sgd", "adam", "adamw"])
def test_state_dict_is_unchanged_by_clip_and_ema(family):
    from iswm_amd import optim

    def make(ps):
        if family == "sgd":
            return optim.FusedSGD(ps, momentum=0.9, nesterov=True, weight_decay=1e-4)
        return (optim.FusedAdam if family == "adam" else optim.FusedAdamW)(ps, weight_decay=1e-2)
    plain, ext = make(_params()), make(_params())
    ext.set_grad_clip(1.0)
    ext.enable_ema(0.99)
    a, b = plain.state_dict(), ext.state_dict()
    assert list(a) == list(b) and a["param_groups"] == b["param_groups"]
    assert list(a["state"]) == list(b["state"])
    for k in a["state"]:
        assert list(a["state"][k]) == list(b["state"][k])
        for name, v in a["state"][k].items():
            assert torch.equal(v, b["state"][k][name])
    assert ext.ema_enabled and not plain.ema_enabled and plain.last_grad_norm is None


def test_set_grad_clip_and_enable_ema_refusals():
    from iswm_amd import optim
    opt = optim.FusedSGD(_params(), momentum=0.9)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            opt.set_grad_clip(bad)
    opt.set_grad_clip(2.0)
    assert opt._max_norm == 2.0
    for off in (None, 0, 0.0):
        opt.set_grad_clip(off)
        assert opt._max_norm is None
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            opt.enable_ema(bad)
    with pytest.raises(RuntimeError):
        with opt.ema_weights():
            pass
    with pytest.raises(RuntimeError):
        opt.ema_state_dict(torch.nn.Linear(1, 1))


def test_ema_state_dict_names_and_roundtrip():
    """on a CPU arena (no kernel runs): names as in model.state_dict(), parameters only, detached copies, load restores them"""
    from iswm_amd import optim
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4))
    opt = optim.FusedSGD(model.parameters(), momentum=0.9)
    opt.enable_ema(0.9, warmup=False)
    sd = opt.ema_state_dict(model)
    assert list(sd) == ["decay", "warmup", "num_updates", "params"] and (sd["decay"], sd["warmup"], sd["num_updates"]) == (0.9, False, 0)
    assert list(sd["params"]) == [k for k, _ in model.named_parameters()]
    assert not set(sd["params"]) & {k for k, _ in model.named_buffers()}
    for k, p in model.named_parameters():
        assert torch.equal(sd["params"][k], p.detach()) and sd["params"][k].data_ptr() != p.data_ptr()
        assert not sd["params"][k].requires_grad
    sd["params"]["0.weight"] = sd["params"]["0.weight"] + 1
    sd["num_updates"] = 6
    other = optim.FusedSGD(model.parameters(), momentum=0.9)        # the same arena, EMA not enabled yet
    other.load_ema_state_dict(model, sd)
    back = other.ema_state_dict(model)
    assert back["num_updates"] == 6 and back["decay"] == 0.9 and back["warmup"] is False
    for k in sd["params"]:
        assert torch.equal(back["params"][k], sd["params"][k])
    del sd["params"]["1.bias"]
    with pytest.raises(KeyError, match="1.bias"):
        other.load_ema_state_dict(model, sd)
    with pytest.raises(ValueError):
        other.ema_state_dict(torch.nn.Linear(3, 4))
