"""The gradient and the optimiser state of the learning update (include/nmpc_policy.h), seen through
nmpc_policy_get_opt_state / nmpc_policy_set_opt_state.

tests/test_gpu_policy.py sees theta after Adam has divided the gradient by its own magnitude: after the first step every
entry has moved by lr * sign(g), whatever |g| is.  Here the gradient itself is read back -- after one step from the reset
state the first moment is (1 - 0.9f) g -- and held, block by block, to the float64 oracle; Adam's update is checked in
isolation from moments put in through the ABI; and the promises of the header about the state (reset by set_params, left
alone by forward and loss, enough to resume a run bit for bit) are checked as written.

Bars.  Gradient blocks: max(1e-5, 4 x the deviation of the float32 oracle from the float64 oracle on the same inputs), the
project's standing rule, for the max-norm and for the relative L2 deviation of every block.  Everything else is counted in
roundings of fp32 and written down where it is asserted.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from tests.solve_helpers import policy_pair

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LR = 1e-3
F32 = np.float32
B1, B2 = F32(0.9), F32(0.999)                   # the kernel's constants, as fp32
C1, C2 = F32(1) - B1, F32(1) - B2               # exact in fp32 (Sterbenz)
EPS = F32(1e-8)

# (n_in, n_out, L, hidden, batch_norm, B): one per dispatch branch of the step
SHAPES = [
    (64, 64, 2, 128, True, 128),      # the 16 B load path in all three GEMM forms; split-K grows to 8, one 16-wide slice per split
    (47, 12, 3, 512, True, 256),      # the reference's network
    (5, 3, 1, 7, True, 2),            # B = 2: 30 of the 32 row chunks are empty
    (9, 4, 2, 65, False, 33),         # no BatchNorm; a one-row split and an empty split
    (9, 4, 2, 65, False, 1),          # B = 1
    (130, 70, 2, 100, True, 129),     # two N tiles in the output layer; a K tail past two KS x BK steps
    (12, 3, 2, 520, True, 40),        # 4 x 520^2 floats exceed the split workspace: two splits, the second short
    (8, 2, 2, 1024, False, 16),       # the workspace cap takes the splits down to one
    (6, 2, 16, 8, True, 9),           # 16 hidden layers: the whole offset table of the Adam kernel
    (8, 256, 1, 32, True, 16),        # the widest output the sign bins hold
    (8, 1, 1, 32, True, 16),          # the narrowest
]
ids = lambda s: "-".join(str(int(v)) for v in s)


def on(pol, a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=pol.device)


def host(pol):
    """theta, running_mean, running_var of the device, as numpy"""
    return [t.cpu().numpy() for t in pol.get_parameters()]


def opt_state(pol):
    m, v, step = pol.get_optimizer_state()
    return m.cpu().numpy(), v.cpu().numpy(), step


def device_gradient(pol, X, Y):
    """The gradient of the L1 loss of (X, Y) at the policy's current parameters, as the device computes it: reset Adam, take
    one step, read the first moment -- m1 = (1 - 0.9f) g, so g = m1 / (1 - 0.9f) to 1 ulp.  The policy is left one Adam step
    (at LR) further.  Returns (g, m, v) as numpy fp32."""
    pol.set_parameters(*pol.get_parameters())
    pol.train_step(X, Y, LR)
    m, v, step = opt_state(pol)
    assert step == 1
    return m / C1, m, v


def blocks(pol):
    """[(name, slice, is a bias in front of a BatchNorm)] of theta"""
    L, bn = pol.dims[2], pol.dims[4]
    return [(name, slice(off, off + int(np.prod(shape))), bool(bn and name.endswith(".b") and int(name.split(".")[1]) < L))
            for name, shape, off in pol.items]


def deviation(a, b):
    """(max |a - b| / max |b|, relative L2) over a block"""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)), float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def batch(shape, seed=5):
    n_in, n_out, L, hidden, bn, B = shape
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, n_in)).astype(F32), rng.standard_normal((B, n_out)).astype(F32)


# Shapes whose noise blocks (test b) are bounded by the float64 oracle's B * 2^-23 * sum_m |dz[m, f]| instead of 4 x the float32
# oracle's largest entry.  On 8-wide blocks that largest entry is the maximum of eight rounding residues of which one to three
# are exactly zero, and it jumps from layer to layer of this one network: 9.5e-6, 9.5e-7, 1.1e-6, 8.6e-8, 2.9e-7 in layers
# 2 .. 6 at the initial parameters (CPU, before any device run); a second fp32 arrangement of the same formula in numpy gives
# 0.3 to 6.6 times the oracle's figure on these blocks, 0.7 to 1.4 times on blocks of 32 features and more.  The other
# shapes keep the float32 oracle's figure -- B = 2 has to: there dz is itself what cancellation leaves (xhat = +-1), and the
# float32 oracle exceeds B * 2^-23 * sum |dz| by a factor of 5000.
NOISE_BY_DZ = {(6, 2, 16, 8, True, 9)}

_cases = {}


def case(shape):
    """The device's gradient and both oracles' at two points -- the parameters of policy_pair and the parameters one Adam step later,
    the oracles loaded with the device's fp32 theta and running statistics at each -- made once per shape and left unchanged:
    (blocks, [{g, v: device; g64, g32: oracles; margin: the smallest |ReLU input| of the float64 oracle}, ...])"""
    if shape not in _cases:
        from oracle.policy_oracle import PolicyOracle
        n_in, n_out, L, hidden, bn, B = shape
        pol, o64 = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
        o32 = PolicyOracle(n_in, n_out, L, hidden, bn, F32)
        X, Y = batch(shape)
        x, y = on(pol, X), on(pol, Y)
        points = []
        for _ in range(2):
            th, rm, rv = host(pol)
            for o in (o64, o32):
                o.theta[:] = th; o.running_mean[:] = rm; o.running_var[:] = rv
            cache = []
            o64.forward(X.astype(np.float64), train=True, cache=cache, update_running=False)
            margin = min(float(np.abs(c[3]).min()) for c in cache[:-1])
            dz = {}
            _, g64, _ = o64.loss_and_grad(X.astype(np.float64), Y.astype(np.float64), dz=dz)
            _, g32, _ = o32.loss_and_grad(X, Y)
            dz = [np.abs(dz[l]).sum(0) for l in range(L)]             # sum over the batch of |dz[m, f]| per hidden layer
            g, _, v = device_gradient(pol, x, y)                      # ... and on to the second point
            points.append(dict(g=g, v=v, g64=g64, g32=g32.astype(np.float64), margin=margin, dz=dz))
        _cases[shape] = (blocks(pol), points)
    return _cases[shape]


# ---------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_gradient_matches_the_float64_oracle_block_by_block(shape):
    """Every W, b, gamma, beta block of every layer, at the initial parameters and one Adam step later; both deviations under
    max(1e-5, 4 x the float32 oracle's).  The biases in front of a BatchNorm (exact gradient zero) are test b's.  A ReLU input
    within rounding of zero would make the gradient itself ambiguous: the smallest one of the float64 oracle is printed.
    The second moment must have seen the same gradient: v = (1 - 0.999f) g^2 within 6 x 2^-24 relative (g carries the two
    roundings of m1 and of the division, twice through the square; v its own two products) and one denormal step."""
    blks, points = case(shape)
    bad = []
    for point, c in enumerate(points):
        print(f"{ids(shape)} point {point}: smallest |ReLU input| of the float64 oracle {c['margin']:.2e}")
        for name, sl, noise in blks:
            if noise:
                continue
            dmax, dl2 = deviation(c["g"][sl], c["g64"][sl])
            omax, ol2 = deviation(c["g32"][sl], c["g64"][sl])
            bar_max, bar_l2 = max(1e-5, 4 * omax), max(1e-5, 4 * ol2)
            print(f"  {name:>12}: device max {dmax:.2e} L2 {dl2:.2e} | float32 oracle max {omax:.2e} L2 {ol2:.2e} | bars {bar_max:.1e} {bar_l2:.1e}"
                  f" | max |g_ref| {np.abs(c['g64'][sl]).max():.2e}")
            if not (dmax < bar_max and dl2 < bar_l2):
                bad.append((point, name, dmax, dl2, bar_max, bar_l2))
        g = c["g"].astype(np.float64)
        v_ref = float(C2) * g * g
        excess = np.abs(c["v"].astype(np.float64) - v_ref) - (6 * 2.0 ** -24 * v_ref + 2.0 ** -149)
        print(f"  v against (1 - 0.999f) g^2: worst {float((np.abs(c['v'] - v_ref) / np.maximum(v_ref, 1e-300)).max()) / 2.0 ** -24:.2f} x 2^-24 relative")
        if excess.max() > 0:
            bad.append((point, "v", int(excess.argmax()), float(excess.max())))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[4]], ids=ids)
def test_bias_gradients_in_front_of_a_batchnorm_are_rounding_noise(shape):
    """Exact gradient zero (the float64 oracle gives ~1e-18); what the device leaves there is rounding noise, bounded per
    entry by 4 x the largest entry the float32 oracle produces for the same block on the same inputs -- noise against noise.
    Where the float32 oracle's own figure is erratic (NOISE_BY_DZ, with the reasons), per entry by B * 2^-23 * sum_m |dz[m, f]|
    of the float64 oracle instead; the float32 oracle's figure is still printed.
    Measured on an MI355X: device 0.37 to 1.6 times the float32 oracle's figure on the ten blocks-of-32-and-more and B = 2
    shapes (2.6e-10 .. 2.5e-8; 2.2e-7 at B = 2); at 16 layers x 8 features 0.19 to 7.7 times it (1.4e-8 .. 1.7e-6), and at most 0.45 of the
    float64 bound per entry."""
    n_in, n_out, L, hidden, bn, B = shape
    blks, points = case(shape)
    bad = []
    for point, c in enumerate(points):
        for name, sl, noise in blks:
            if not noise:
                continue
            got, ref32, ref64 = (float(np.abs(c[k][sl]).max()) for k in ("g", "g32", "g64"))
            line = f"{ids(shape)} point {point} {name:>10}: device max |g| {got:.2e} | float32 oracle {ref32:.2e} | float64 oracle {ref64:.1e}"
            if shape in NOISE_BY_DZ:
                bound = B * 2.0 ** -23 * c["dz"][int(name.split(".")[1])]
                ratio = float((np.abs(c["g"][sl]) / bound).max())
                print(line + f" | B 2^-23 sum|dz| {bound.min():.2e} .. {bound.max():.2e}, worst entry at {ratio:.3f} of its bound")
                if not ratio <= 1.0:
                    bad.append((point, name, ratio))
            else:
                print(line)
                if not got <= 4 * ref32:
                    bad.append((point, name, got, ref32))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("shape", [(9, 12, 2, 65, True, 34), (130, 70, 2, 100, True, 130)], ids=ids)
def test_output_bias_gradient_counts_signs_exactly(shape):
    """The output bias gradient is an integer count of signs over B * n_out.  Targets placed at prediction +-1 in equal numbers
    per column give exactly 0.0; with exact ties (sign 0) and unequal numbers the first moment of the bias is
    float32(0.1f * count / (B * n_out)) within 1 ulp (the device rounds the quotient, then the product)."""
    n_in, n_out, L, hidden, bn, B = shape
    X, Y = batch(shape)
    twin, _ = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
    _, pred = twin.train_step(on(twin, X), on(twin, Y), LR, return_pred=True)
    pred = pred.cpu().numpy()
    assert B % 2 == 0
    rng = np.random.default_rng(2)
    balanced = np.tile(np.where(np.arange(B) % 2 == 0, 1.0, -1.0).astype(F32)[:, None], (1, n_out))
    ragged = rng.choice(np.array([1.0, -1.0, 0.0], F32), size=(B, n_out), p=[0.45, 0.3, 0.25])
    for what, s in (("balanced", balanced), ("ties", ragged)):
        pol, _ = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
        target = pred + s                                            # s = 0: the prediction itself, bit for bit
        assert np.array_equal(np.sign(pred - target), -np.sign(s))
        loss, again = pol.train_step(on(pol, X), on(pol, target), LR, return_pred=True)
        assert np.array_equal(again.cpu().numpy(), pred)             # an identical policy: the same prediction
        m, _, _ = opt_state(pol)
        got = m[blocks(pol)[-1][1]]
        count = -s.astype(np.float64).sum(0)
        want = (float(C1) * count / (B * n_out)).astype(F32)
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want))
        print(f"{ids(shape)} {what}: counts {count.min():.0f} .. {count.max():.0f}, m of the output bias within {ulps.max():.2f} ulp")
        if what == "balanced":
            assert not count.any() and np.array_equal(got, np.zeros(n_out, F32)), got
        else:
            assert count.any() and len(np.unique(count)) > 3 and (ragged == 0).sum() > n_out
            assert ulps.max() <= 1.0, (got, want)


# ---------------------------------------------------------------------------------------------- d
_adam = {}


def adam_case():
    """One policy, its parameters, a batch and the gradient terms of that batch from a twin in the reset state: the twin's
    moments after one step are fl((1 - 0.9f) g) and fl(fl((1 - 0.999f) g) g) exactly, whatever the compiler contracts (the
    other product is with zero).  Run-to-run bit equality of the gradient is tests/test_gpu_policy.py's."""
    if not _adam:
        shape = (130, 70, 2, 100, True, 129)
        n_in, n_out, L, hidden, bn, B = shape
        X, Y = batch(shape, seed=8)
        pol, _ = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
        twin, _ = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
        params = host(pol)
        _, gm, gv = device_gradient(twin, on(twin, X), on(twin, Y))
        _adam.update(pol=pol, params=params, x=on(pol, X), y=on(pol, Y), gm=gm, gv=gv)
    return _adam


@pytest.mark.parametrize("t0", [0, 1, 9, 999, 100000])
def test_adam_update_from_given_moments(t0):
    """m, v random with |m| and sqrt(v) log-uniform in [1e-6, 1], step = t0; one step on a fixed batch.
    m', v': within 2 ulp of the fp32 restatement fl(fl(b m) + term) (a contracted multiply-add skips the rounding of one
    product).
    theta': against the float64 formula on the device's (m', v', t0 + 1) with the fp32 constants: 16 x 2^-24 |update| +
    ulp(theta) / 2.  The bias corrections 1 - b^t are formed in fp32 and lose digits to cancellation at small t, which that
    count of roundings leaves out, so the fp32 numpy restatement of the update is measured against the float64 formula as
    well; only where its largest relative deviation exceeds 16 x 2^-24 does 4 x that deviation take its place.
    Measured on an MI355X: m' bit-equal, v' within 1 ulp; the device's update off by 3.5, 60, 6.0, 3.0, 2.7 x 2^-24 at t0 = 0, 1, 9,
    999, 100000, the restatement by 3.7, 61, 6.1, 3.5, 3.4: only t0 = 1 takes the wider bar (243 x 2^-24)."""
    c = adam_case()
    pol, gm, gv = c["pol"], c["gm"], c["gv"]
    rng = np.random.default_rng(100 + t0)
    n = pol.n_theta
    m0 = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 0, n)).astype(F32)
    v0 = ((10.0 ** rng.uniform(-6, 0, n)) ** 2).astype(F32)
    pol.set_parameters(*c["params"])
    pol.set_optimizer_state(m0, v0, t0)
    m_in, v_in, step_in = opt_state(pol)
    assert np.array_equal(m_in, m0) and np.array_equal(v_in, v0) and step_in == t0
    pol.train_step(c["x"], c["y"], LR)
    m1, v1, step = opt_state(pol)
    theta1 = host(pol)[0]
    assert step == t0 + 1
    # the moments
    am, av = B1 * m0, B2 * v0                                        # fp32 products
    m_ref, v_ref = am + gm, av + gv
    tol_m, tol_v = 2 * np.spacing(np.abs(m_ref)), 2 * np.spacing(v_ref)
    em, ev = np.abs(m1.astype(np.float64) - m_ref), np.abs(v1.astype(np.float64) - v_ref)
    print(f"t0 = {t0}: m' within {float((em / tol_m).max()) * 2:.2f} ulp, v' within {float((ev / tol_v).max()) * 2:.2f} ulp of the restatement")
    assert (em <= tol_m).all() and (ev <= tol_v).all()
    # the update
    t = t0 + 1
    m64, v64, theta0 = m1.astype(np.float64), v1.astype(np.float64), c["params"][0].astype(np.float64)
    upd64 = float(F32(LR)) * (m64 / (1.0 - float(B1) ** t)) / (np.sqrt(v64 / (1.0 - float(B2) ** t)) + float(EPS))
    c1, c2 = F32(1) - np.power(B1, F32(t), dtype=F32), F32(1) - np.power(B2, F32(t), dtype=F32)
    upd32 = F32(LR) * (m1 / c1) / (np.sqrt(v1 / c2) + EPS)
    assert upd32.dtype == F32
    own = float((np.abs(upd32.astype(np.float64) - upd64) / np.abs(upd64)).max())
    rel = 4 * own if own > 16 * 2.0 ** -24 else 16 * 2.0 ** -24
    want = theta0 - upd64
    bar = rel * np.abs(upd64) + 0.5 * np.spacing(np.maximum(np.abs(theta0), np.abs(want)).astype(F32)).astype(np.float64)
    err = np.abs(theta1.astype(np.float64) - want)
    half_ulp = bar - rel * np.abs(upd64)
    dev_rel = float((np.maximum(err - half_ulp, 0) / np.abs(upd64)).max())      # what the rounding of theta' cannot account for
    print(f"t0 = {t0}: the fp32 restatement of the update deviates by {own / 2.0 ** -24:.1f} x 2^-24 relative -> bar {rel / 2.0 ** -24:.1f} x 2^-24 |update|"
          f" + ulp/2; device: update off by at least {dev_rel / 2.0 ** -24:.2f} x 2^-24, worst error / bar {float((err / bar).max()):.3f}, c1 {c1:.9g} c2 {c2:.9g}")
    assert (err <= bar).all(), (int((err > bar).sum()), float((err / bar).max()))


# ---------------------------------------------------------------------------------------------- e
def everything(pol):
    return host(pol) + list(opt_state(pol))


def assert_identical(a, b, what):
    for name, p, q in zip(("theta", "running_mean", "running_var", "m", "v", "step"), a, b):
        assert np.array_equal(p, q), (what, name)


def test_set_parameters_resets_and_forward_and_loss_leave_the_state_alone():
    shape = (9, 4, 2, 65, True, 33)
    n_in, n_out, L, hidden, bn, B = shape
    pol, _ = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
    m, v, step = opt_state(pol)
    assert step == 0 and not m.any() and not v.any()                 # a fresh policy
    X, Y = batch(shape)
    x, y = on(pol, X), on(pol, Y)
    for _ in range(3):
        pol.train_step(x, y, LR)
    before = everything(pol)
    assert before[5] == 3 and before[3].any() and (before[4] > 0).any()
    pol.forward(x); pol.loss(x, y); pol.forward(x[:1].contiguous()); pol.loss(x[:5].contiguous(), y[:5].contiguous())
    assert_identical(before, everything(pol), "forward and loss")
    pol.set_parameters(*pol.get_parameters())
    m, v, step = opt_state(pol)
    assert step == 0 and not m.any() and not v.any()
    # step 0 with zero moments is the state set_parameters leaves: the next step is the same either way
    other, _ = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
    other.set_parameters(*pol.get_parameters())
    other.set_optimizer_state(before[3], before[4], 7)
    other.set_optimizer_state(np.zeros(pol.n_theta, F32), np.zeros(pol.n_theta, F32), 0)
    la, lb = pol.train_step(x, y, LR), other.train_step(x, y, LR)
    assert torch.equal(la, lb)
    assert_identical(everything(pol), everything(other), "reset by hand")


@pytest.mark.parametrize("shape", [(9, 4, 2, 65, False, 33), (47, 12, 3, 512, True, 256)], ids=ids)
def test_resume_from_saved_state_is_bit_identical(shape):
    """3 steps, parameters and optimiser state into a fresh DevicePolicy, 2 more steps == 5 uninterrupted steps: theta, running
    statistics, m, v, step and losses."""
    from iterative_learning_nmpc_amd.policy import DevicePolicy
    n_in, n_out, L, hidden, bn, B = shape
    rng = np.random.default_rng(11)
    whole, _ = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
    first, _ = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
    X = on(whole, rng.standard_normal((5, B, n_in))); Y = on(whole, rng.standard_normal((5, B, n_out)))
    losses = [whole.train_step(X[s], Y[s], LR).item() for s in range(5)]
    resumed = [first.train_step(X[s], Y[s], LR).item() for s in range(3)]
    second = DevicePolicy(n_in, n_out, L, hidden, bn, batch_max=B, seed=None)
    second.set_parameters(*first.get_parameters())
    second.set_optimizer_state(*first.get_optimizer_state())
    assert_identical(everything(first), everything(second), "the copy")
    del first
    resumed += [second.train_step(X[s], Y[s], LR).item() for s in range(3, 5)]
    assert resumed == losses, (resumed, losses)
    assert_identical(everything(whole), everything(second), "5 steps against 3 + 2")
    assert second.get_optimizer_state()[2] == 5


def test_refused_optimizer_state_leaves_the_handle_usable():
    import ctypes
    from iterative_learning_nmpc_amd._lib import NmpcError, ptr, stream
    shape = (9, 4, 2, 65, False, 33)
    n_in, n_out, L, hidden, bn, B = shape
    pol, _ = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
    twin, _ = policy_pair(n_in, n_out, L, hidden, bn, batch_max=B)
    X, Y = batch(shape)
    x, y = on(pol, X), on(pol, Y)
    pol.train_step(x, y, LR); twin.train_step(x, y, LR)
    before = everything(pol)
    m, v = on(pol, before[3]), on(pol, before[4])
    with pytest.raises(NmpcError, match=r"\(-1\).*step >= 0"):
        pol.set_optimizer_state(m, v, -1)
    assert b"step" in pol.lib.nmpc_policy_last_error(pol._h)
    for bad_m, bad_v in ((m[:-1], v), (m, torch.cat([v, v])), (m[:0], v[:0])):
        with pytest.raises(ValueError, match="elements"):
            pol.set_optimizer_state(bad_m, bad_v, 2)
    # the library's own refusals: null moments
    for args in ((None, ptr(v)), (ptr(m), None)):
        assert pol.lib.nmpc_policy_set_opt_state(pol._h, *args, 2, stream(pol.device)) == -1
        assert b"null" in pol.lib.nmpc_policy_last_error(pol._h)
    # get: any of the three may be missing; the step alone comes back without a device copy
    step = ctypes.c_longlong(-5)
    assert pol.lib.nmpc_policy_get_opt_state(pol._h, None, None, ctypes.byref(step), stream(pol.device)) == 0 and step.value == 1
    only_v = torch.zeros_like(v)
    assert pol.lib.nmpc_policy_get_opt_state(pol._h, None, ptr(only_v), None, stream(pol.device)) == 0
    assert np.array_equal(only_v.cpu().numpy(), before[4])
    assert_identical(before, everything(pol), "after the refusals")
    la, lb = pol.train_step(x, y, LR), twin.train_step(x, y, LR)
    assert torch.equal(la, lb)
    assert_identical(everything(pol), everything(twin), "the next step")
