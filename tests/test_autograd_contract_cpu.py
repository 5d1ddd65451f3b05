"""The bookkeeping behind the autograd contract (iswm_amd/network/_hip.py: new_serial, keep, peek, take, claim, drop, once) on
plain objects and parameter-free nn.Modules: no GPU, no kernel.  What the modules do with it on the device is
tests/test_autograd_contract_gpu.py."""
import threading

import pytest
import torch
import torch.nn as nn

from iswm_amd.network import _hip


class Plain(object):
    """any object will do for keep / take: they only use the two attributes"""
    pass


class Sink(object):
    def __init__(self, serial):
        self.serial = serial


class Node(nn.Module):
    def __init__(self, *children):
        super().__init__()
        self.kids = nn.ModuleList(children)


def test_serials_grow_and_are_distinct_across_threads():
    a, b = _hip.new_serial(), _hip.new_serial()
    assert isinstance(a, int) and 0 < a < b
    got = []
    ts = [threading.Thread(target=lambda: got.extend(_hip.new_serial() for _ in range(200))) for _ in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert len(set(got)) == 800 and min(got) > b


def test_matching_serial_returns_the_payload_and_clears():
    m, s = Plain(), _hip.new_serial()
    payload = ("x", 3)
    _hip.keep(m, s, payload)
    assert _hip.peek(m, Sink(s)) is payload and m._saved is payload          # peek leaves it in place
    assert _hip.take(m, Sink(s)) is payload
    assert m._saved is None and _hip.peek(m, Sink(s)) is None


def test_a_call_lists_its_modules_and_the_modules_hold_plain_ints():
    """the Serial carries the modules that kept state for it; a module's stamp is a plain int (no reference cycle through
    the call), equal to the Serial"""
    a, b, s = Plain(), Plain(), _hip.new_serial()
    _hip.keep(a, s, ("a",))
    _hip.keep(b, s, ("b",))
    _hip.keep(Plain(), False, ("c",))
    assert s.mods == [a, b] and type(a._stamp) is int and a._stamp == s and isinstance(s, int) and s


def test_newer_stamp_is_replaced():
    m = Plain()
    a, b = _hip.new_serial(), _hip.new_serial()
    _hip.keep(m, a, ("a",))
    _hip.keep(m, b, ("b",))
    assert _hip.peek(m, Sink(a)) is None
    with pytest.raises(RuntimeError, match="replaced the state saved for this backward") as e:
        _hip.take(m, Sink(a))
    assert "Plain" in str(e.value) and "run forward and backward of each batch in turn" in str(e.value)
    assert m._saved is None                                                  # dropped: nothing stale is left behind


def test_empty_is_consumed():
    m, s = Plain(), _hip.new_serial()
    _hip.keep(m, s, ("a",))
    _hip.take(m, Sink(s))
    with pytest.raises(RuntimeError, match="already consumed") as e:
        _hip.take(m, Sink(s))
    assert "Plain" in str(e.value) and "retain_graph" in str(e.value)
    with pytest.raises(RuntimeError, match="already consumed"):              # a module no forward went through
        _hip.take(Plain(), Sink(None))


@pytest.mark.parametrize("falsy", [False, 0, None])
def test_falsy_save_stores_nothing_and_clears(falsy):
    m, s = Plain(), _hip.new_serial()
    _hip.keep(m, s, ("a",))
    _hip.keep(m, falsy, ("b",))
    assert m._saved is None
    with pytest.raises(RuntimeError, match="replaced"):                      # the forward in between is seen, not "consumed"
        _hip.take(m, Sink(s))


def test_by_hand_save_true_is_unchecked_but_never_a_type_error():
    m = Plain()
    _hip.keep(m, True, ("a",))
    assert _hip.take(m, _hip.GradSink()) == ("a",)                           # GradSink() carries no serial
    _hip.keep(m, True, ("b",))
    assert _hip.take(m, None) == ("b",)                                      # nor does a missing sink
    with pytest.raises(RuntimeError, match="consumed"):
        _hip.take(m, None)
    assert _hip.GradSink(serial=7).serial == 7 and _hip.GradSink().serial is None


def test_claim_passes_on_the_calls_own_state_and_ignores_modules_that_did_not_run():
    leaf, idle = Node(), Node()
    root = Node(leaf, idle)
    old, s = _hip.new_serial(), _hip.new_serial()
    _hip.keep(idle, old, ("stale",))                                         # ran in an earlier call only
    _hip.keep(leaf, s, ("l",))
    _hip.keep(root, s, ("r",))
    _hip.claim(root, s)
    assert leaf._saved == ("l",) and root._saved == ("r",) and idle._saved == ("stale",)


def test_claim_replaced_by_a_child_forward_names_both_classes_and_drops():
    class Leaf(Node):
        pass
    leaf = Leaf()
    root = Node(Node(leaf))
    s = _hip.new_serial()
    for m in root.modules():
        _hip.keep(m, s, ("p",))
    later = _hip.new_serial()
    _hip.keep(leaf, later, ("later",))                                       # the child run on its own, saving
    with pytest.raises(RuntimeError, match="replaced") as e:
        _hip.claim(root, s)
    assert "Node" in str(e.value) and "Leaf" in str(e.value)
    assert all(m._saved is None for m in root.modules())
    with pytest.raises(RuntimeError, match="replaced"):                      # also what the later call's own backward is told
        _hip.claim(leaf, later)
    s2 = _hip.new_serial()                                                   # usable again
    for m in root.modules():
        _hip.keep(m, s2, ("q",))
    _hip.claim(root, s2)
    assert _hip.take(leaf, Sink(s2)) == ("q",)


def test_claim_replaced_by_a_forward_that_saved_nothing():
    leaf = Node()
    root = Node(leaf)
    s = _hip.new_serial()
    for m in root.modules():
        _hip.keep(m, s, ("p",))
    _hip.keep(leaf, False, None)
    with pytest.raises(RuntimeError, match="replaced"):
        _hip.claim(root, s)


def test_claim_consumed_after_the_state_was_taken():
    leaf = Node()
    root = Node(leaf)
    s = _hip.new_serial()
    for m in root.modules():
        _hip.keep(m, s, ("p",))
    _hip.claim(root, s)
    for m in root.modules():
        _hip.take(m, Sink(s))
    with pytest.raises(RuntimeError, match="consumed") as e:
        _hip.claim(root, s)
    assert "Node" in str(e.value)


def test_distinct_roots_do_not_disturb_each_other():
    r1, r2 = Node(Node()), Node(Node())
    s1 = _hip.new_serial()
    for m in r1.modules():
        _hip.keep(m, s1, ("one",))
    s2 = _hip.new_serial()
    for m in r2.modules():
        _hip.keep(m, s2, ("two",))
    for m in r2.modules():
        _hip.keep(m, False, None)
    _hip.claim(r1, s1)
    assert all(_hip.take(m, Sink(s1)) == ("one",) for m in r1.modules())


class _Sum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.sum()

    @staticmethod
    @_hip.once
    def backward(ctx, g):
        return g.expand(3)


def test_once_refuses_create_graph_and_leaves_plain_backward_alone():
    x = torch.ones(3, requires_grad=True)
    with pytest.raises(RuntimeError, match="once_differentiable") as e:
        torch.autograd.grad(_Sum.apply(x), x, create_graph=True)
    assert "_Sum" in str(e.value)
    with pytest.raises(RuntimeError, match="once_differentiable"):           # the upstream gradient itself requires grad
        torch.autograd.grad(_Sum.apply(x) ** 2, x, create_graph=True)
    (2 * _Sum.apply(x)).backward()
    assert torch.equal(x.grad, torch.full((3,), 2.0))


def test_every_backward_of_the_package_is_once():
    """the bridges and the criteria: a decorated backward carries functools.wraps' __wrapped__"""
    from iswm_amd.network import _deeplab, utils
    from iswm_amd.utils import loss
    fns = [_hip._Bridge, utils._SegBridge, _deeplab._HeadBridge, _deeplab._V3Bridge, loss._LossFn, loss._OverlapLossFn,
           loss._OhemLossFn, loss._LovaszLossFn]
    for f in fns:
        assert hasattr(f.backward, "__wrapped__"), f.__name__


def test_loss_fn_refuses_a_second_backward_before_touching_its_tensor():
    """_LossFn.backward on a stand-in ctx: the refusal comes before the saved gradient is read or rescaled"""
    from iswm_amd.utils import loss

    class Ctx(object):
        consumed, mode = True, 0

        @property
        def saved_tensors(self):
            raise AssertionError("read after the call was consumed")
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CrossEntropyLoss: .*already consumed"):
            loss._LossFn.backward(Ctx(), torch.ones(()))
        Ctx.mode = 2
        with pytest.raises(RuntimeError, match="FocalLoss: .*already consumed"):
            loss._LossFn.backward(Ctx(), torch.ones(()))
