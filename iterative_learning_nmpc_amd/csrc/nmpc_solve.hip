// nmpc_solve.hip -- batched NMPC solve on gfx950: two kernels per SQP iteration (one in the two-wave variant, which
// linearises inside the QP kernel: qp_linearizes_itself).
//
// Replaces the reference's per-step solve (mpc_controller/utils/solver.py:396-403 ->
// acados SQP / HPIPM):
//   nmpc_linearize_kernel  one thread per (problem, stage): dynamics, analytic A,B, defects,
//                          gradients, constraint values -> workspace (fully parallel, any
//                          register budget, no cross-lane traffic)
//   nmpc_qp_kernel         one problem per wavefront: interior-point loop of Riccati sweeps
//        phase R (serial stages)  backward sweep on 16x16 tiles: MFMA products + readlane LDL'
//        phase F (serial stages)  rollout of the closed loop (row-per-lane VALU mat-vec)
//        phase I (lane = stage)   interior-point step: slacks, multipliers, fraction to boundary
//        phase S (lane = stage)   step (optionally l1-merit backtracking), status, write back
// Splitting the linearisation off keeps the sweep kernel's register allocation small (the
// Jacobian code wants hundreds of VGPRs; fused, it forced the MFMA accumulators of the sweeps
// through AGPR<->VGPR copies and pinned the kernel at one wave per SIMD).
// Stage matrices A~, B~, K~, Acl~ live in an HBM/L2 workspace as compact images (640-768 B);
// trajectories, gradients and IPM state of a problem live in LDS (39.9 KB at N = 50) inside
// nmpc_qp_kernel -- or, in its lean variant for batches beyond one wave per SIMD, partly in the workspace (Lds).
// Kernel variants (template flags): LDS layout, precision of the barrier product, set of contact
// patterns with a static stage body.  DESIGN.md 5 has the measurements behind each choice.
// By file: nmpc_solve_layout.hpp (argument block, images, workspace and LDS layouts: what the host and the other families read),
// nmpc_linearize.hip.inc (linearize_node and its kernel), nmpc_qp.hip.inc (the QP kernel).  linearize_node comes first because the
// two-wave QP kernel calls it; the order of the kernels in the code object is set where they are named (launch_qp in nmpc_api.hip).
#include "nmpc_solve_layout.hpp"
#include "nmpc_linearize.hip.inc"
#include "nmpc_qp.hip.inc"
