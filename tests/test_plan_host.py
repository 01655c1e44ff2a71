"""CPU tests of the sampling-plan codec (papc_amd/plan.py) and of the compact / lists policy (compact.StackPolicy): every layout sample() can
return, built from small CPU tensors of the right shapes and dtypes, with the expected fields stated here, not re-derived through the codec."""
import itertools

import pytest
import torch

from papc_amd import _lib
from papc_amd import compact as C
from papc_amd.layers import PointNetSetAbstraction, PointNetSetAbstractionMsg
from papc_amd.plan import N_COMPACT, N_LISTS, N_XYZ_PRE, Cursor, Level, new_xyz

B, N, S = 2, 16, 4
G = B * S


def _same(a, b):
    return len(a) == len(b) and all(x is y for x, y in zip(a, b))


def _head(Ks):
    return (torch.zeros(B, S, 3),) + tuple(torch.zeros(B, S, K, dtype=torch.int32) for K in Ks)


def _xyz_pre(K):
    return (torch.zeros(G * K, 4), torch.zeros(16, dtype=torch.float64))


def test_slot_counts_are_those_of_the_plan_classes():
    assert (N_COMPACT, N_LISTS, N_XYZ_PRE) == (7, 3, 2)
    assert len(C.alloc(G, 4, "cpu")) == N_COMPACT and len(C.alloc_lists(B, N, G, 4, "cpu")) == N_LISTS
    assert C.is_lists(C.alloc_lists(B, N, G, 4, "cpu"))
    cap = C.alloc_lists(B, N, G, 4, "cpu")[1].shape[0]
    assert C.is_lists((torch.zeros(B * N, 2, dtype=torch.int32), torch.zeros(cap, dtype=torch.int32), torch.zeros(cap, 4)))   # a caller's pmeta of cap rows
    assert not C.is_lists(C.alloc(G, 4, "cpu")[:3]) and not C.is_lists(C.alloc_lists(B, N, G, 4, "cpu")[:2]) and not C.is_lists(())
    pr, pw, pm = C.alloc_lists(B, N, G, 4, "cpu")
    assert not C.is_lists((pr.float(), pw, pm)) and not C.is_lists((pr, pw, pm.double())) and not C.is_lists((pr, pw, pm[:, :3]))
    assert not C.is_lists((pr[:, 0], pw, pm))


@pytest.mark.parametrize("length", [2, 4, 5, 9, 12])
def test_ssg_layouts(length):
    K = 4
    head = _head([K])
    pre = _xyz_pre(K) if length == 4 else None
    cp = C.alloc(G, K, "cpu") if length in (9, 12) else None
    pl = C.alloc_lists(B, N, G, K, "cpu") if length in (5, 12) else None
    flat = head + (pre or ()) + (cp or ()) + (pl or ())
    assert len(flat) == length
    lv = Level.parse(list(flat), G, [K])                   # (any sequence: a copy that kept nothing but the tensors)
    assert lv.new_xyz is flat[0] and new_xyz(flat) is flat[0] and _same(lv.idxs, [flat[1]])
    assert (lv.xyz_pre is None) if pre is None else _same(lv.xyz_pre, pre)
    if cp is None:
        assert lv.cplans == [None]
    else:
        assert _same(lv.cplans[0].tensors(), cp) and (lv.cplans[0].G, lv.cplans[0].K) == (G, K)
        # what bench.py reads: a compacted SSG level has 9 or 12 tensors and element 4 is ``rows``
        assert len(flat) in (9, 12) and lv.cplans[0].rows is flat[4] and tuple(flat[4].shape) == (2,)
    if pl is None:
        assert lv.plists == [None]
    else:
        assert _same(lv.plists[0].tensors(), pl) and lv.plists[0].compact == (cp is not None) and lv.plists[0].pmom is not None
    assert _same(lv.flat(), flat) and isinstance(lv.flat(), tuple)
    assert _same(lv.branch(0), (cp or ()) + (pl or ()))

    # sample(out=flat) in the same mode: every piece gets its own buffers back
    w = Cursor(flat)
    assert _same(w.next(2), head)
    w.put(*head)
    if length == 4:
        assert _same(w.next(N_XYZ_PRE), pre)
        assert _same(w.put(*pre), flat)
        return
    got = w.next(N_COMPACT, then=(0, N_LISTS))
    assert (got is None) if cp is None else _same(got, cp)
    w.put(*(cp or ()))
    got = w.next(N_LISTS, then=(0,))
    assert (got is None) if pl is None else _same(got, pl)
    assert _same(w.put(*(pl or ())), flat)


def test_cursor_gives_nothing_that_belongs_to_another_piece():
    K = 4
    head, cp, pl = _head([K]), C.alloc(G, K, "cpu"), C.alloc_lists(B, N, G, K, "cpu")
    w = Cursor(None)
    assert w.next(2) is None and w.put(*head) == head and w.next(N_COMPACT, then=(0, N_LISTS)) is None and w.next(N_LISTS, then=(0,)) is None
    # a compacted plan's buffers for a layer that now runs padded: its lists are made afresh (the 3 tensors after idx are compact tensors)
    w = Cursor(head + cp + pl)
    w.put(*head)
    assert _same(w.next(N_COMPACT, then=(0, N_LISTS)), cp) and w.next(N_LISTS, then=(0,)) is None
    # a padded plan's buffers for a layer that now runs compacted: nothing fits
    w = Cursor(head + pl)
    w.put(*head)
    assert w.next(N_COMPACT, then=(0, N_LISTS)) is None
    w.put(*cp)
    assert w.next(N_LISTS, then=(0,)) is None
    # an evaluation plan's buffers (no lists) for a training layer: compact plan in place, lists afresh
    w = Cursor(head + cp)
    w.put(*head)
    assert _same(w.next(N_COMPACT, then=(0, N_LISTS)), cp)
    w.put(*cp)
    assert w.next(N_LISTS, then=(0,)) is None
    # a coordinates-only level wants at least its two tensors after (new_xyz, idx)
    w = Cursor(head + _xyz_pre(K)[:1])
    w.put(*head)
    assert w.next(N_XYZ_PRE) is None


@pytest.mark.parametrize("length", [1, 3, 6, 7, 8, 10, 11, 13])
def test_ssg_wrong_length_is_rejected(length):
    K = 4
    flat = (_head([K]) + C.alloc(G, K, "cpu") + C.alloc_lists(B, N, G, K, "cpu") + (torch.zeros(1),))[:length]
    with pytest.raises(ValueError, match="sampling plan of %d tensors" % length):
        Level.parse(flat, G, [K])


def test_ssg_three_tensors_that_are_no_lists_are_rejected():
    K = 4
    with pytest.raises(ValueError, match="sampling plan of 5 tensors"):
        Level.parse(_head([K]) + C.alloc(G, K, "cpu")[:3], G, [K])


def _msg_cases():
    for Ks in ([4, 8], [4, 8, 16]):
        for flags in itertools.product([False, True], repeat=len(Ks)):
            for lists in ((False, True) if any(flags) else (False,)):
                yield pytest.param(Ks, flags, lists, id="R%d-%s-%s" % (len(Ks), "".join("c" if f else "p" for f in flags), "lists" if lists else "nolists"))


@pytest.mark.parametrize("Ks,flags,lists", list(_msg_cases()))
def test_msg_layouts(Ks, flags, lists):
    R = len(Ks)
    head = _head(Ks)
    cps = [C.alloc(G, K, "cpu") if f else None for K, f in zip(Ks, flags)]
    pls = [C.alloc_lists(B, N, G, K, "cpu") if (f and lists) else None for K, f in zip(Ks, flags)]
    flat = head
    for cp, pl in zip(cps, pls):
        flat = flat + (cp or ()) + (pl or ())
    assert len(flat) == 1 + R + N_COMPACT * sum(flags) + N_LISTS * sum(flags) * lists
    lv = Level.parse(tuple(flat), G, Ks, compacted=list(flags))
    assert lv.new_xyz is head[0] and _same(lv.idxs, head[1:]) and lv.xyz_pre is None
    for i in range(R):
        if cps[i] is None:
            assert lv.cplans[i] is None and lv.plists[i] is None and lv.branch(i) == ()
            continue
        assert _same(lv.cplans[i].tensors(), cps[i]) and (lv.cplans[i].G, lv.cplans[i].K) == (G, Ks[i])
        if lists:
            assert _same(lv.plists[i].tensors(), pls[i]) and lv.plists[i].compact is True
        else:
            assert lv.plists[i] is None
        assert _same(lv.branch(i), cps[i] + (pls[i] or ()))
    assert _same(lv.flat(), flat)

    # sample(out=flat) in the same mode
    w = Cursor(flat)
    assert _same(w.next(1 + R), head)
    w.put(*head)
    for i in range(R):
        if cps[i] is not None:
            assert _same(w.next(N_COMPACT), cps[i])
            w.put(*cps[i])
            if lists:
                assert _same(w.next(N_LISTS), pls[i])
                w.put(*pls[i])
    assert _same(w.res, flat)

    # a tensor too few, one too many, or a layout for other branches than the layer runs compacted: no silent misreading
    if any(flags):
        with pytest.raises(ValueError, match="sampling plan of %d tensors" % (len(flat) - 1)):
            Level.parse(flat[:-1], G, Ks, compacted=list(flags))
        with pytest.raises(ValueError, match="sampling plan"):
            Level.parse(flat, G, Ks, compacted=[False] * R)
    with pytest.raises(ValueError, match="sampling plan of %d tensors" % (len(flat) + 1)):
        Level.parse(flat + (torch.zeros(1),), G, Ks, compacted=list(flags))
    with pytest.raises(ValueError, match="sampling plan of %d tensors" % R):
        Level.parse(flat[:R], G, Ks, compacted=list(flags))


# ---- the compact / lists policy ----

class _FakePlan:
    def __init__(self, frac):
        self.frac = frac

    def fraction(self):
        return self.frac


@pytest.fixture
def kernels(monkeypatch):
    """the two library calls the policy makes, replaced: every stack has its compacted flavour, a plan reports the fraction set here"""
    state = {"ok": True, "frac": 0.5, "outs": []}
    monkeypatch.setattr(C, "stack_ok", lambda M, K, couts: state["ok"])

    def fake_plan(idx, out=None):
        state["outs"].append(out)
        return _FakePlan(state["frac"])
    monkeypatch.setattr(C, "plan", fake_plan)
    monkeypatch.setattr(C, "POLICY", "auto")
    monkeypatch.setattr(C, "LISTS", 2)
    return state


def _ssg(D=128, **kw):
    return PointNetSetAbstraction(128, 0.4, 64, D + 3, [128, 128, 256], False, **kw)


def _msg(D=128, **kw):
    return PointNetSetAbstractionMsg(128, [0.4, 0.8], [64, 128], D, [[128, 128, 256], [128, 196, 256]], **kw)


IDX = torch.zeros(8, 128, 64, dtype=torch.int32)


def test_policy_forced_and_measured(kernels):
    ssg, msg = _ssg(), _msg()
    for pol in [ssg._policy] + msg._policies:
        assert pol.on is None and pol.mode(8) == "probe"
    assert ssg._compact_on is None and msg._compact_on == {}
    # forced on: a plan without a measurement; the MSG branch records it (its forward reads the layout from the flag), the SSG layer does not
    ssg.compact = msg.compact = True
    assert ssg._policy.mode(8) is True and ssg._policy.plan(IDX) is not None and ssg._compact_on is None
    assert msg._policies[1].mode(8) is True and msg._policies[1].plan(IDX) is not None and msg._compact_on == {1: True}
    # forced off
    ssg.compact = msg.compact = False
    assert ssg._policy.mode(8) is None and ssg._policy.plan(IDX) is None
    assert msg._policies[0].mode(8) is None and msg._policies[0].plan(IDX) is None and msg._compact_on == {1: True}
    # undecided: measured once, kept
    ssg.compact = msg.compact = None
    assert ssg._policy.mode(8) == "probe"                      # (forcing left no trace on the SSG layer)
    assert msg._policies[1].mode(8) is True and msg._policies[0].mode(8) == "probe"
    bufs = tuple(range(N_COMPACT))
    kernels["frac"] = C.AUTO_MAX_FRACTION
    assert ssg._policy.plan(IDX, out=bufs) is not None and kernels["outs"][-1] is bufs and ssg._compact_on is True and ssg._policy.mode(8) is True
    kernels["frac"] = 0.9
    assert ssg._policy.plan(IDX) is not None and ssg._compact_on is True          # decided: not measured again
    full = _ssg()
    assert full._policy.plan(IDX) is None and full._compact_on is False and full._policy.mode(8) is False and full._policy.plan(IDX) is None
    assert msg._policies[0].plan(IDX) is None and msg._compact_on == {0: False, 1: True}
    # PAPC_COMPACT=1 forces like compact = True; a stack without the kernels' compacted flavour stays padded whatever is forced
    kernels["frac"] = 0.5
    C.POLICY = "1"
    assert full._policy.mode(8) is True and _ssg()._policy.mode(8) is True
    kernels["ok"] = False
    ssg.compact = True
    assert ssg._policy.mode(8) is None and ssg._policy.plan(IDX) is None


def test_policy_does_not_measure_inside_a_capture(kernels, monkeypatch):
    monkeypatch.setattr(_lib, "_capturing", lambda: True)
    ssg, msg = _ssg(), _msg()
    assert ssg._policy.plan(IDX) is None and ssg._compact_on is None and msg._policies[0].plan(IDX) is None and msg._compact_on == {}
    assert kernels["outs"] == []                                 # nothing was launched
    ssg.compact = True                                          # forced or decided: no host read needed
    assert ssg._policy.plan(IDX) is not None


def test_policy_width_and_group_all(kernels):
    # SSG tests the feature width as it is, MSG the width its branches pad to
    for D, ssg_ok, msg_ok in [(128, True, True), (16, True, True), (12, False, False), (13, False, True), (18, False, True), (3, False, False),
                              (0, False, False)]:
        assert (_ssg(D)._policy.mode(8) is not None) == ssg_ok, D
        assert (_msg(D)._policies[0].mode(8) is not None) == msg_ok, D
        assert bool(_ssg(D)._policy.wants_lists(False, 512)) == ssg_ok and bool(_msg(D)._policies[0].wants_lists(True, 512)) == msg_ok
    one = PointNetSetAbstraction(128, 0.4, 64, 131, [128], False)          # a single layer: no gather-add first layer + max layer pair
    assert one._policy.mode(8) is None
    ga = PointNetSetAbstraction(None, None, None, 259, [256, 512, 1024], True)
    ga.compact = True
    assert ga._policy.mode(8) is None and ga._policy.plan(IDX) is None and not ga._policy.wants_lists(False, 128)


@pytest.mark.parametrize("lists,ssg_padded,ssg_compacted,msg_compacted", [(0, False, False, False), (1, False, True, True), (2, True, True, True)])
def test_policy_lists(kernels, monkeypatch, lists, ssg_padded, ssg_compacted, msg_compacted):
    monkeypatch.setattr(C, "LISTS", lists)
    ssg, msg = _ssg(), _msg()
    assert bool(ssg._policy.wants_lists(False, 512)) == ssg_padded and bool(ssg._policy.wants_lists(True, 512)) == ssg_compacted
    assert bool(msg._policies[0].wants_lists(True, 512)) == msg_compacted
    assert not msg._policies[0].wants_lists(False, 512)         # MSG: only ever for a compacted branch
    # only for a training layer that keeps the gather gradients, over clouds the builder can hold
    assert not ssg._policy.wants_lists(True, C.MAX_LIST_POINTS + 1) and not msg._policies[0].wants_lists(True, C.MAX_LIST_POINTS + 1)
    assert bool(ssg._policy.wants_lists(True, C.MAX_LIST_POINTS)) == ssg_compacted
    ssg.eval(), msg.eval()
    assert not ssg._policy.wants_lists(True, 512) and not msg._policies[0].wants_lists(True, 512)
    assert not _ssg(reference_quirks=True)._policy.wants_lists(True, 512) and not _msg(reference_quirks=True)._policies[0].wants_lists(True, 512)
