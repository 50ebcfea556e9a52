"""GPU checks of the push on nmpc_contact_step_batch (nmpc_contact_set_push) against tests/push_reference.py (itself checked in
tests/test_push_reference.py).

The accuracy bar is the contact plant's own (`torque_helpers.held`): a device result is compared with the fp64 reference under
    max(1e-5 * scale, 4 x the deviation of the numpy-float32 run of the same reference loop from the fp64 run),
both computed here, never from the code under test.  Bit-for-bit claims are equality of the bit patterns.  Every figure is
printed before it is asserted.  The window starts and ends inside the call: first_substep is no multiple of n_sub."""
import copy

import numpy as np
import pytest

from tests import contact_reference as cr
from tests import fd_reference as fr
from tests import push_reference as pr
from tests.plant_helpers import DT, KD, KP, NAMES, detached  # noqa: F401
from tests.torque_helpers import Case, bar, general_case, ground, held, host, layer, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_SUB, FIRST, COUNT = 4, 1, 2                                       # the window [1, 3) of four substeps
# tree -> (B, pushed joint): B = 33 leaves the last robot alone in a second block of 32; the 32-joint tree runs 16 robots per
# block, B = 17 is one block and a robot.  Joint 9 of that tree and joint 7 of tree23 are bodies inside the tree; joint 9 has
# prismatic joints on its path to the root.
TREES = {"quadruped": (33, 5), "tree23": (33, 7), "tree32": (17, 9)}


class PushRun:
    """B robots of a tree through pushed_step_ref and contact_step_ref, in fp64 over fd_ref and in numpy float32 over aba"""
    def __init__(self, name):
        B, self.joint = TREES[name]
        self.c = c = {"quadruped": lambda: Case(fr.quadruped(), B, seed=333), "tree23": lambda: general_case(fr.random_tree(), B, 7),
                      "tree32": lambda: general_case(fr.random_tree(n=32, seed=14, feet=(4, 31, 31, 17)), B, 8)}[name]()
        m, rng = c.m, np.random.default_rng(90)
        self.F = rng.uniform(-80, 80, (B, 3)).astype(np.float32)
        self.q_des = (c.q[:, m.n - m.nu:] + rng.uniform(-0.1, 0.1, (B, m.nu))).astype(np.float32)
        run = lambda **kw: [np.stack(x) for x in zip(*[pr.pushed_step_ref(m, c.g, c.q[b], c.v[b], DT, N_SUB, c.tau[b], self.q_des[b], KP, KD,  # noqa: E731
                                                                           self.F[b], self.joint, FIRST, COUNT, **kw) for b in range(B)])]
        self.ref, self.f32 = run(), run(fd=fr.aba, dtype=np.float32)
        self.plain = [np.stack(x) for x in zip(*[cr.contact_step_ref(m, c.g, c.q[b], c.v[b], DT, N_SUB, c.tau[b], self.q_des[b], KP, KD)
                                                 for b in range(B)])]

    def device(self, B=None, n_sub=N_SUB, q=None, v=None):
        c, s = self.c, slice(0, B)
        return c.L.contact_step(c.q[s] if q is None else q, c.v[s] if v is None else v, DT, n_sub, tau_ff=c.tau[s], q_des=self.q_des[s],
                                kp=KP, kd=KD, ground=ground(c.g))


class Runs(dict):
    def __missing__(self, name):
        self[name] = PushRun(name)
        return self[name]


@pytest.fixture(scope="module")
def runs():
    return Runs()


CASES = [("quadruped", 1), ("quadruped", 33), ("tree23", 33), ("tree32", 17)]


@pytest.mark.parametrize("tree,B", CASES)
def test_the_pushed_step_matches_the_reference(runs, detached, tree, B):
    r = runs[tree]
    L = r.c.L
    # without the push in the reference the test could pass with the push ignored: it moves v_out by more than 100 bars
    moved, b_v = np.abs(r.ref[1][:B] - r.plain[1][:B]).max(), bar(r.ref[1][:B], r.f32[1][:B])
    print(f"{tree} B {B}: the push moves v_out by {moved:.3e}, its bar is {b_v:.3e} (ratio {moved / b_v:.1f})")
    assert moved > 100 * b_v
    L.set_push(torch.as_tensor(r.F, device=L.device), FIRST, COUNT, joint=r.joint)
    got = host(*r.device(B))
    n, nf = r.c.m.n, len(r.c.m.foot_joint)
    assert [x.shape for x in got] == [(B, n)] * 3 + [(B, nf, 3), (B, r.c.m.nu)]
    assert all([held(name, x, ref[:B], f32[:B]) for name, x, ref, f32 in zip(NAMES, got, r.ref, r.f32)])


@pytest.mark.parametrize("tree,B", CASES)
def test_outside_the_window_and_detached_are_the_unpushed_bits(runs, detached, tree, B):
    r = runs[tree]
    L = r.c.L
    F = torch.as_tensor(r.F, device=L.device)
    plain = r.device(B)
    for first, count in ((N_SUB, 3), (-7, 7), (2, 0)):
        L.set_push(F, first, count, joint=r.joint)
        assert all(same(x, y) for x, y in zip(r.device(B), plain)), (first, count)
    L.set_push(F, FIRST, COUNT, joint=r.joint)
    pushed = r.device(B)
    assert not same(pushed[1], plain[1])
    L.set_push(None)
    assert all(same(x, y) for x, y in zip(r.device(B), plain))


@pytest.mark.parametrize("tree,B", CASES)
def test_one_call_is_the_chain_of_single_substeps_with_the_window_moved(runs, detached, tree, B):
    """Substeps 0 and 3 are launches of the un-pushed kernel in the one call and in the chain, substeps 1 and 2 launches of the
    pushed kernel: one launch of two in the call, two launches of one in the chain."""
    r = runs[tree]
    L = r.c.L
    F = torch.as_tensor(r.F, device=L.device)
    L.set_push(F, FIRST, COUNT, joint=r.joint)
    once = r.device(B)
    q, v, out = None, None, None
    for i in range(N_SUB):
        L.set_push(F, FIRST - i, COUNT, joint=r.joint)            # first_substep = 1, 0, -1, -2
        out = r.device(B, n_sub=1, q=q, v=v)
        q, v = out[0], out[1]
    diff = [float((a - b).abs().max()) for a, b in zip(out, once)]
    print(f"{tree} B {B}: largest |chain - one call| of q, v, a, f, tau: {diff}")
    assert all(same(x, y) for x, y in zip(out, once))


def test_refusals(runs, detached):
    import ctypes

    from iterative_learning_nmpc_amd import _lib
    from iterative_learning_nmpc_amd._lib import NmpcError
    r = runs["quadruped"]
    L, c = r.c.L, r.c
    F = torch.as_tensor(r.F, device=L.device)
    text = lambda: L.lib.nmpc_torque_last_error(L._h).decode()      # noqa: E731
    attach = lambda *a: L.lib.nmpc_contact_set_push(L._h, ctypes.byref(_lib.NmpcPushCfg(*a)))      # noqa: E731
    for args, why in (((None, 33, 5, 0, 1), "force is NULL"), ((F.data_ptr(), 0, 5, 0, 1), "force_rows must be at least 1"),
                      ((F.data_ptr(), 33, -1, 0, 1), "joint must be in"), ((F.data_ptr(), 33, 18, 0, 1), "joint must be in"),
                      ((F.data_ptr(), 33, 5, 0, -1), "n_substeps must not be negative")):
        assert attach(*args) == -1 and why in text(), args
    # a refused attachment leaves the layer detached: the step is the un-pushed one
    plain = r.device(8)
    L.set_push(F[:4], FIRST, COUNT)
    # B > force_rows: refused before any launch, the outputs keep their sentinels
    q, v, tau, q_des = (torch.as_tensor(x[:8], device=L.device).contiguous() for x in (c.q, c.v, c.tau, r.q_des))
    outs = [torch.full(s, -77.0, device=L.device) for s in ((8, 18), (8, 18), (8, 18), (8, 4, 3), (8, 12))]
    ptr, cfg, st = _lib.ptr, ground(c.g).cfg(), _lib.stream(L.device)
    rc = L.lib.nmpc_contact_step_batch(L._h, 8, N_SUB, DT, ctypes.byref(cfg), ptr(q), ptr(v), ptr(tau), ptr(q_des), KP, KD, *[ptr(x) for x in outs], st)
    assert rc == -1 and "B exceeds force_rows" in text()
    assert all(bool((x == -77.0).all()) for x in outs)
    A = q_des[:, None, :].contiguous()
    q2, v2 = q.clone(), v.clone()
    with pytest.raises(NmpcError, match="B exceeds force_rows"):
        L.contact_track(q2, v2, A, DT, N_SUB, tau_ff=tau, kp=KP, kd=KD, ground=ground(c.g))
    assert same(q2, q) and same(v2, v)
    # within force_rows the same attachment is taken, and detached the bits are the un-pushed ones again
    assert not same(r.device(4)[1], plain[1][:4])
    L.set_push(None)
    assert all(same(x, y) for x, y in zip(r.device(8), plain))


def test_a_massless_leaf_still_gives_nan_rows(runs, detached):
    r, B = runs["quadruped"], 33
    c = r.c
    bad = copy.deepcopy(c.m)
    bad.mass[17] = 0.0; bad.inertia[17] = 0.0
    Lb = layer(bad)
    Lb.set_push(torch.as_tensor(r.F, device=Lb.device), FIRST, COUNT)
    out = host(*Lb.contact_step(c.q[:B], c.v[:B], DT, N_SUB, tau_ff=c.tau[:B], q_des=r.q_des[:B], kp=KP, kd=KD))
    assert [x.shape for x in out] == [(B, 18)] * 3 + [(B, 4, 3), (B, 12)] and all(np.isnan(x).all() for x in out)
