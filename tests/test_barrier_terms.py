"""The barrier terms of the centroidal QP kernel, G'DG and G'v of the friction pyramids.

The model supplies them in closed form per foot (Centroidal::foot_terms, nmpc_models.hpp): eight numbers, each the fmaf chain
that the fp32 matrix instruction runs for that entry of the product Gs'[Gs | vt].  The CPU test compiles the hook for the host
and compares it, bit for bit, with that chain over the dense M::G.  The GPU tests solve small problems whose contact schedules
reach every place that writes or reads barrier terms (a touch-down, all contact patterns and the run-time fallback, binding
pyramids, no active row at all, several stages per lane, the bf16 product) against the fp64 oracle, and the resident against
the lean kernel variant bit for bit.  The bar is the one of tests/solve_helpers.py (within_tolerance): 1e-5 relative L2, or 1.5 x
the fp32 oracle's own distance from the fp64 one where that is larger -- and at horizons of four or five stages it is larger
(the CPU's own fp32 error on cases (a)-(c) is 1.4e-5 .. 4.7e-5: a short horizon leaves the barrier systems stiff), so each
tensor is held against its own floor."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.solve_helpers import dev, gpu_solve, make_solver, oracle_solve, rel, within_tolerance  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include "nmpc_models.hpp"
using M = nmpc::Centroidal;
static unsigned bits(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
int main() {
    nmpc::ModelParams mp = {};
    unsigned long long rng = 88172645463325252ull;
    auto uni = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (float)((rng >> 11) % 1000003ull) / 1000003.0f; };
    int checked = 0, bad = 0;
    const float mus[3] = {0.3f, 0.7f, 1.0f};
    for (int stance = 0; stance < 16; ++stance)                  // every row subset a stance mask implies
        for (int rep = 0; rep < 40; ++rep) {
            mp.mu = mus[rep % 3];
            float sq[16], vt[16];
            for (int j = 0; j < 16; ++j) {
                const bool on = (stance >> (j & 3)) & 1;
                const float D = std::exp(12.0f * uni() - 6.0f);    // D = lam/s > 0 over five decades
                sq[j] = on ? std::sqrt(D) : 0.0f;
                vt[j] = on ? (2.0f * uni() - 1.0f) * 50.0f : 0.0f;
            }
            // the dense product as the matrix instruction contracts it: step f takes rows row_of(f, 0..3) in order,
            // one fmaf per row, on Gs = G.sq and [Gs | vt]
            float T[12][13];
            for (int m = 0; m < 12; ++m)
                for (int c = 0; c < 13; ++c) {
                    float acc = 0.0f;
                    for (int f = 0; f < 4; ++f)
                        for (int jj = 0; jj < 4; ++jj) {
                            const int row = M::row_of(f, jj);
                            const float a = M::G(mp, row, m) * sq[row];
                            const float b = (c == 12) ? vt[row] : M::G(mp, row, c) * sq[row];
                            acc = std::fmaf(a, b, acc);
                        }
                    T[m][c] = acc;
                }
            for (int f = 0; f < 4; ++f) {
                float o[8];
                M::foot_terms(mp, f, sq, vt, o);
                const int x = 3 * f, y = x + 1, z = x + 2;
                const float want[8] = {T[x][x], T[y][y], T[z][z], T[x][z], T[x][12], T[y][12], T[z][12], T[y][z]};
                for (int i = 0; i < 8; ++i, ++checked)
                    if (bits(o[i]) != bits(want[i])) { ++bad; std::printf("stance %d foot %d term %d: %a != %a\n", stance, f, i, o[i], want[i]); }
                // symmetric, and nothing outside the foot's block: the eight numbers are all there is
                if (bits(T[x][z]) != bits(T[z][x]) || bits(T[y][z]) != bits(T[z][y]) || T[x][y] != 0.0f || T[y][x] != 0.0f) ++bad;
                for (int m = 0; m < 12; ++m)
                    for (int c = x; c <= z; ++c)
                        if (m / 3 != f && (T[m][c] != 0.0f || T[c][m] != 0.0f)) ++bad;
                if (!((stance >> f) & 1))
                    for (int i = 0; i < 8; ++i)
                        if (bits(o[i]) != 0u) ++bad;              // a swing foot: exact (positive) zeros
            }
        }
    std::printf("checked %d bad %d\n", checked, bad);
    return bad ? 1 : 0;
}
"""


def test_foot_terms_equal_the_dense_product_bit_for_bit(tmp_path):
    """Host build of the model's per-foot hook against the k-ordered fmaf chain of the dense Gs'[Gs | vt]: every stance mask,
    random positive D over five decades, three friction coefficients; exact."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "foot_terms.cpp"
    src.write_text(HOST_PROGRAM)
    exe = tmp_path / "foot_terms"
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(ROOT, "iterative_learning_nmpc_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "checked 20480 bad 0" in out.stdout


# ---- small-shape solves ------------------------------------------------------------------------------------------------------
TROT_A, TROT_B, FOUR = [1, 0, 0, 1], [0, 1, 1, 0], [1, 1, 1, 1]
SCHEDULES = {          # stance flags of stage 0 .. N-1 (the terminal node repeats the last stage)
    "a": [TROT_A, TROT_B, FOUR, TROT_A],                       # stage 3 builds the cost tiles of four-foot stage 2: wider
    "b": [[0, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 0], FOUR],       # one foot, flight, three feet
    "d": [[0, 0, 0, 0]] * 3,                                    # no active row: the single non-IPM sweep
}


def scheduled(N, B, seed, schedule=None, mu=None):
    """centroidal_trot with the stance flags of `schedule`, the weight shared by the stance feet as force reference and start"""
    from iterative_learning_nmpc_amd import workloads as wl
    w = wl.centroidal_trot(B=B, N=N, seed=seed)
    if mu is not None:
        w.mp[6] = mu
    if schedule is not None:
        flags = np.asarray(schedule + [schedule[-1]], np.float32)
        assert flags.shape == (N + 1, 4)
        w.params[:, :, 0:4] = flags
        share = (-w.mp[5] * w.mp[1]) / np.maximum(flags[:N].sum(-1), 1.0)
        for i in range(4):
            w.yref[:, :, 12 + 3 * i: 14 + 3 * i] = 0.0
            w.yref[:, :, 14 + 3 * i] = (share * flags[:N, i]).astype(np.float32)
        w.U[:] = w.yref[:, :, 12:]
    return w


def at_the_fp32_floor(name, got, o64, o32):
    """status equal, X and U each within the bar of tests/solve_helpers.py against the fp64 oracle"""
    (X, U, st, _), (X64, U64, st64, _), (X32, U32, _, _) = got, o64, o32
    eX, eU, fX, fU = rel(X, X64), rel(U, U64), rel(X32, X64), rel(U32, U64)
    print(f"{name}: gpu-vs-f64 X {eX:.2e} U {eU:.2e}; f32-vs-f64 floor X {fX:.2e} U {fU:.2e}")
    assert np.array_equal(st, st64)
    assert within_tolerance(eX, fX) and within_tolerance(eU, fU), (eX, eU, fX, fU)


def solve_both_variants(w, B, dev, monkeypatch, all_patterns=None, precision=0):
    out = {}
    for variant in ("resident", "lean"):
        monkeypatch.setenv("NMPC_QP_VARIANT", variant)       # read by nmpc_create
        s = make_solver(w, B, dev, precision=precision, n_ipm=6)
        if all_patterns is not None:
            assert s.set_contact_patterns(all_patterns=all_patterns) == all_patterns
        out[variant] = gpu_solve(s, w)
    for a, b in zip(out["resident"], out["lean"]):
        assert np.array_equal(a, b)
    return out["resident"]


@pytest.mark.gpu
def test_touch_down_to_four_foot_stance(dev, monkeypatch, oracle64, oracle32):
    """(a) N = 4, two diagonal pairs and a touch-down to four-foot stance at stage 2: the stage above it builds cost tiles
    with more stance feet than its own pattern has."""
    w = scheduled(4, 4, seed=3, schedule=SCHEDULES["a"])
    at_the_fp32_floor("touch-down", solve_both_variants(w, 4, dev, monkeypatch), oracle_solve(oracle64, w), oracle_solve(oracle32, w))


@pytest.mark.gpu
@pytest.mark.parametrize("all_patterns", [True, False])
def test_three_foot_one_foot_and_flight_stages(dev, monkeypatch, oracle64, oracle32, all_patterns):
    """(b) N = 4, one stage each of one-foot stance, flight and three-foot stance under a four-foot one: the kernel with a
    static body per pattern and the default kernel's run-time fallback.  The gate of the random-pattern test
    (test_all_contact_patterns_kernel_matches_default_and_oracle, 3e-5), or the fp32 oracle's own floor where that is beyond
    the gate: measured X 2.57e-5 / 1.94e-5 (all patterns / fallback; fp32 oracle 1.38e-5), U 4.54e-5 / 4.64e-5 (fp32 oracle
    4.74e-5) -- the same figures before and after the barrier terms moved (the kernels are bit-identical).
    What this gate can see: the bound in force on U is 1.5 x 4.74e-5 = 7.1e-5, so a wrong pattern, a missing foot or a wrong
    stage is caught, a last-bit error in one barrier term is not -- no oracle gate at a four-stage horizon could, its fp32
    floor is above the project's bar.  Last bits are guarded by the host chain test above, by resident == lean below (the lean
    kernel still forms the matrix product) and by the byte comparison of bench.py --dump-outputs between builds."""
    w = scheduled(4, 4, seed=0, schedule=SCHEDULES["b"])
    X, U, st, _ = solve_both_variants(w, 4, dev, monkeypatch, all_patterns=all_patterns)
    (X64, U64, st64, _), (X32, U32, _, _) = oracle_solve(oracle64, w), oracle_solve(oracle32, w)
    eX, eU, fX, fU = rel(X, X64), rel(U, U64), rel(X32, X64), rel(U32, U64)
    print(f"patterns all={all_patterns}: gpu-vs-f64 X {eX:.2e} U {eU:.2e}; f32-vs-f64 floor X {fX:.2e} U {fU:.2e}")
    assert np.array_equal(st, st64)
    assert (eX < 3e-5 or within_tolerance(eX, fX)) and (eU < 3e-5 or within_tolerance(eU, fU)), (eX, eU, fX, fU)


@pytest.mark.gpu
def test_binding_pyramids(dev, monkeypatch, oracle64, oracle32):
    """(c) N = 5 at mu = 0.3 (test_centroidal_active_friction): the barrier terms dominate Huu."""
    w = scheduled(5, 4, seed=1, mu=0.3)
    got, o64 = solve_both_variants(w, 4, dev, monkeypatch), oracle_solve(oracle64, w)
    at_the_fp32_floor("binding pyramids", got, o64, oracle_solve(oracle32, w))
    stance = w.params[:, :5, :4]

    def pyramid_use(U):      # max(|fx|, |fy|) / (mu fz) of the stance feet: 1 on a face of the pyramid
        f = np.asarray(U, np.float64).reshape(4, 5, 4, 3)
        return np.abs(f[..., :2]).max(-1) / (0.3 * np.maximum(f[..., 2], 1e-9)) * stance
    use64, use = pyramid_use(o64[1]), pyramid_use(got[1])
    print(f"binding pyramids: largest use of a pyramid, oracle {use64.max():.3f} device {use.max():.3f}")
    # a pyramid binds (the interior point stays inside: 0.95 in the fp64 oracle, as the box of test_double_integrator_box_constraints at 0.9),
    # on the device at the same feet, and none is violated
    assert use64.max() > 0.9 and np.array_equal(use > 0.9, use64 > 0.9) and use.max() < 1.0 + 1e-4


@pytest.mark.gpu
def test_all_flight_takes_the_plain_sweep(dev, monkeypatch, oracle64):
    """(d) N = 3, every foot in the air at every stage: n_act == 0, one sweep without barrier terms."""
    w = scheduled(3, 4, seed=7, schedule=SCHEDULES["d"])
    X, U, st, _ = solve_both_variants(w, 4, dev, monkeypatch)
    X64, U64, st64, _ = oracle_solve(oracle64, w)
    print(f"flight: X {rel(X, X64):.2e} U {rel(U, U64):.2e}")
    assert np.array_equal(st, st64)
    assert rel(X, X64) < 1e-5 and rel(U, U64) < 1e-5, (rel(X, X64), rel(U, U64))


def test_oracles_agree_at_sixty_six_stages(oracle64, oracle32):
    """The reference of case (e) on its own: fp32 and fp64 oracle within the gate at N = 66."""
    w = scheduled(66, 2, seed=11)
    X64, U64, st64, _ = oracle_solve(oracle64, w)
    X32, U32, st32, _ = oracle_solve(oracle32, w)
    assert np.array_equal(st32, st64)
    assert rel(X32, X64) < 1e-5 and rel(U32, U64) < 1e-5, (rel(X32, X64), rel(U32, U64))


@pytest.mark.gpu
def test_several_stages_per_lane(dev, monkeypatch, oracle64, oracle32):
    """(e) N = 66, B = 2: the start-of-iteration coefficient loop writes the barrier terms of every interior-point iteration
    and the update runs in two passes."""
    w = scheduled(66, 2, seed=11)
    at_the_fp32_floor("N = 66", solve_both_variants(w, 2, dev, monkeypatch), oracle_solve(oracle64, w), oracle_solve(oracle32, w))


@pytest.mark.gpu
def test_bf16_barrier_product_did_not_move(dev, monkeypatch, golden_dir):
    """(f) case (a) at precision = 1: bit-identical to the stored output of the kernel before the fp32 barrier terms moved
    (tests/golden/barrier_terms_bf16_case_a.npz, written on an MI355X by the parent of that change)."""
    w = scheduled(4, 4, seed=3, schedule=SCHEDULES["a"])
    X, U, st, stats = solve_both_variants(w, 4, dev, monkeypatch, precision=1)
    g = np.load(os.path.join(golden_dir, "barrier_terms_bf16_case_a.npz"))
    assert np.array_equal(X, g["X"]) and np.array_equal(U, g["U"]) and np.array_equal(st, g["status"]) and np.array_equal(stats, g["stats"])
