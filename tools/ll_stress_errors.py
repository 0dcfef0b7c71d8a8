"""The low-level CLF-QP kernel on the stress cases of tests/ll_cases.py, against the extended-precision
reference (tests/ll_reference.py) and the fp64 oracle: the table of profiles/ll_stress_errors.txt.

    python tools/ll_stress_errors.py [--lib libsrbnmpc_<tag>.so] [case ...]

Needs a GPU.  Per case: the rows active at the reference's final point (agents of 24 with a friction /
torque / CLF row at its bound), E_orc (the oracle's worst distance from the reference over the compared
iterates, max|x - x_ref| / max(1, |x_ref|_inf)), the bound of tests/test_ll_gpu_stress.py, the kernel's worst
trajectory error (same measure), its final-point error where kernel and reference are both OPTIMAL (same
measure, and absolute next to the oracle's absolute one and the tests' bound on it), and the exits: agents where reference and oracle
disagree on (status, iters), how many of those the kernel shares with each, agents whose exit is neither's,
agents where the kernel / the oracle end at MAXIT (the reference never does).
"""
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (ROOT, os.path.join(ROOT, "srb-cbf-nmpc_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ll_cases  # noqa: E402


def main():
    args = sys.argv[1:]
    lib = "libsrbnmpc.so"
    if args[:1] == ["--lib"]:
        lib = args[1]
        args = args[2:]
        import srbnmpc
        srbnmpc.use_library(lib)
    names = args or list(ll_cases.CASES)
    print(f"# srb_ll_kernel ({lib}) on tests/ll_cases.py, 24 agents a case; tools/ll_stress_errors.py")
    print("# fric/torq/clf: agents with a row of the family within 1e-6 of its bound at the reference's final point")
    print("# E_orc, gpu_traj, gpu_fin: max|x - x_ref| / max(1, |x_ref|_inf); gpu_abs, orc_abs: max|x - x_ref| at the final point,\n# bnd_abs = max(1e-8, 10 orc_abs) the tests' bound on gpu_abs")
    print("# split: agents where reference and oracle differ in (status, iters); =ref / =orc: whose exit the kernel has there;")
    print("# neither: agents whose exit is neither's; gpu@max / orc@max: agents ending at MAXIT (the reference: none)")
    print(f"{'case':<13}{'fric':>5}{'torq':>5}{'clf':>4}{'E_orc':>9}{'bound':>9}{'gpu_traj':>9}{'gpu_fin':>9}{'gpu_abs':>9}"
          f"{'orc_abs':>9}{'bnd_abs':>9}{'split':>6}{'=ref':>5}{'=orc':>5}{'neither':>8}{'gpu@max':>8}{'orc@max':>8}")
    for n in names:
        t, e = ll_cases.trajectories(n), ll_cases.gpu_errors(n)
        act = t["active"]
        gmax = int((ll_cases.gpu_runs(n)[-1]["status"] == 2).sum())
        print(f"{n:<13}{act['friction'].sum():>5}{act['torque'].sum():>5}{act['clf'].sum():>4}{e['E_orc']:>9.1e}"
              f"{max(1e-8, 10 * e['E_orc']):>9.1e}{e['e_traj']:>9.1e}{e['e_final_rel']:>9.1e}{e['e_final']:>9.1e}"
              f"{e['orc_final']:>9.1e}{ll_cases.final_bound(n):>9.1e}{e['split']:>6}{e['with_ref']:>5}{e['with_orc']:>5}{e['neither']:>8}{gmax:>8}"
              f"{e['orc_stall']:>8}", flush=True)


if __name__ == "__main__":
    main()
