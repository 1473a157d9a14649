"""The memory-map bodies under AddressSanitizer and UBSan, as a stand-alone program: tests/native/mg_memory_main.cpp (a `main`
around tests/native/mg_memory.cpp and mg_explore.cpp) compiled with g++ -fsanitize=address,undefined -fno-sanitize-recover=all,
the sanitizers' runtimes linked into the executable (-static-libasan -static-libubsan), and run as a child process in the
environment it inherits — random grids, agent records and hide tables from a seed, W and H from 1 to 40 and 255, views 3 to 31,
one-, 64- and 256-lane workgroups, every plane, table and scratch block of the exact size.  A dword stored past a pair's plane,
a table read past the object list or a shift by the word width ends the program.  Nothing sanitized is loaded into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_sanitized_program(tmp_path):
    prog = str(tmp_path / "mg_memory_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "marlgrid_amd", "csrc"),
                           "-I", os.path.join(HERE, "native"), os.path.join(HERE, "native", "mg_memory_main.cpp"), "-o", prog])
    out = subprocess.run([prog, "11", "180"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "ok 180"
