"""csrc/mrbo_lane_tables.h compiled alone with the host compiler for every input dimension d = 1..16
and both fantasy capacities: LaneTables<D, FMAX> carries a static_assert that every word of the
lane index table unpacks to the Gram pair, the Hessian pair and the (row, column) of its own index, so
a wrong table does not compile -- here also for the dimensions the default library does not build.
A second translation unit with a deliberately wrong expectation shows that the compile does check."""
import os
import shutil
import subprocess

import conftest

CSRC = os.path.join(conftest.PKG, "csrc")
# a host C++17 compiler: g++ / c++, else the clang++ of the ROCm that builds the library
CXX = (shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
       or shutil.which("/opt/rocm/llvm/bin/clang++"))


def compile_only(tmp_path, name, body):
    assert CXX is not None, "no host C++ compiler (g++, c++, clang++)"
    src = tmp_path / name
    src.write_text('#include "mrbo_lane_tables.h"\n' + body)
    return subprocess.run([CXX, "-std=c++17", "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True)


def test_tables_compile_for_every_dimension_and_capacity(tmp_path):
    body = "".join(f"template struct mrbo::LaneTables<{d}, {f}>;\n" for d in range(1, 17) for f in (4, 6))
    # spot values of the generator itself: the (D+1)² triangle at d = 2 is (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    body += "static_assert(mrbo::tri_unrank(3, 3).a == 1 && mrbo::tri_unrank(3, 3).b == 1, \"\");\n"
    body += "static_assert(mrbo::tri_unrank(3, 5).a == 2 && mrbo::tri_unrank(3, 5).b == 2, \"\");\n"
    body += "static_assert(mrbo::tri_unrank(7, 27).a == 6 && mrbo::tri_unrank(7, 27).b == 6, \"\");\n"
    body += "static_assert(mrbo::LaneTables<6, 4>::NT == 28 && mrbo::LaneTables<16, 6>::NT == 153, \"\");\n"
    r = compile_only(tmp_path, "ok.cpp", body)
    assert r.returncode == 0, r.stderr


def test_a_wrong_expectation_does_not_compile(tmp_path):
    r = compile_only(tmp_path, "bad.cpp", "static_assert(mrbo::tri_unrank(3, 3).a == 0, \"moved\");\n")
    assert r.returncode != 0 and "moved" in r.stderr
