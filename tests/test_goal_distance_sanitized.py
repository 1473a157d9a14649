"""The goal-distance bodies under AddressSanitizer and UBSan, as a stand-alone program: tests/native/mg_goal_dist_main.cpp (a
`main` around tests/native/mg_goal_dist.cpp) compiled with g++ -fsanitize=address,undefined -fno-sanitize-recover=all, the
sanitizers' runtimes linked into the executable (-static-libasan -static-libubsan), and run as a child process in the environment
it inherits — random grids from a seed, W and H from 1 to 70 and H in {64, 65, 128, 255}, the general path at 64 lanes and at 1
and the register-resident path against a queue search, with result buffers of the exact size.  A shift by the word width, a word
read past a plane or a field entry stored past an env's rows ends the program.  Nothing sanitized is loaded into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_sanitized_program(tmp_path):
    prog = str(tmp_path / "mg_goal_dist_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "marlgrid_amd", "csrc"), "-I", os.path.join(HERE, "native"),
                           os.path.join(HERE, "native", "mg_goal_dist_main.cpp"), "-o", prog])
    out = subprocess.run([prog, "7", "280"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "ok 280"
