"""The carver of athena_amd/csrc/pieces.h on the host: tests/fixtures/pieces_main.cpp carves arrays of every element size out of a
std::vector<char>, writes every byte, and holds bytes() to the arithmetic of the carvers it replaced.  Built with the address and
undefined-behaviour sanitizers where a one-line program links with them, without them otherwise; no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build(src, out, flags):
    return subprocess.run([CXX, "-std=c++17", "-g", "-Wall", *flags, "-I", os.path.join(ROOT, "athena_amd", "csrc"), str(src), "-o",
                           str(out)], capture_output=True, text=True)


def test_pieces_host_program(tmp_path):
    assert CXX, "no C++ compiler"
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = _build(probe, tmp_path / "probe", SANITIZE)
    flags = SANITIZE if p.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0 else []
    exe = tmp_path / "pieces_main"
    b = _build(os.path.join(ROOT, "tests", "fixtures", "pieces_main.cpp"), exe, flags)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "pieces: ok"
