"""The per-trip slot-kind tables of csrc/srb_kernel_params.h (srb_trip_kinds / srb_trip_rows / srb_trip_all_rows_on,
which the compiled-shape solve and polish kernels specialise their slot passes by) against the run-time rule
slot -> kind, for every (trip, lane) of the three compiled shapes, and "any kind, two rows" for a run-time shape:
a stand-alone g++ program (tests/cpp/slot_kinds_check.cpp), no GPU.  A kind missing from a trip's mask would drop
that slot's constraint rows without any error at run time."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "slot_kinds_check.cpp")


def test_trip_tables_cover_the_run_time_rule(tmp_path):
    exe = str(tmp_path / "slot_kinds_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function",
                    "-I", os.path.join(ROOT, "srb-cbf-nmpc_amd", "csrc"), SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "slot kinds ok" in r.stdout, r.stdout + r.stderr
