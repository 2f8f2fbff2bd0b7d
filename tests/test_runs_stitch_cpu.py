"""CPU: the host scan between the two passes of the run kernels (panagram_amd/csrc/pg_runs_host.h: runs_stitch) held to a brute-force
loop by tools/runs_stitch_check.cpp, compiled without sanitizer flags and run; and the one field order of a chunk's counts."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "panagram_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_runs_stitch_check_program(tmp_path):
    exe = str(tmp_path / "runs_stitch_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tools", "runs_stitch_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("ok:"), (p.returncode, p.stdout, p.stderr)


def test_the_shared_pieces_stand_once():
    """the predecessor exchange of the run scan, the fold's turns and the scan of the chunks' counts: one copy each"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC)}
    # (pg_novel.hip keeps the run scan's loop written out, for the measured reason beside it)
    assert [f for f, t in src.items() if "__shfl_up" in t and f in ("pg_synteny.hip", "pg_locate.hip")] == []
    assert "__shfl_up" in src["pg_runscan.h"] and "written out" in src["pg_novel.hip"]
    assert sum(len(re.findall(r"constexpr uint32_t \w*FOLD_TURNS\b", t)) for t in src.values()) == 1
    assert [f for f, t in src.items() if re.search(r"block_add\([^;]*;\s*__syncthreads\(\);\s*block_add\(", t)] == []
    assert [f for f, t in src.items() if "runs_stitch(" in t and f.startswith("pg_api")] == []  # (through runs_two_pass only)
