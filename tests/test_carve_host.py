"""The block layout rule of host_common.h -- plan a block's bytes from its layout, then carve it with the same layout -- in a stand-alone host program
under the sanitizers (tests/hostcheck/carve_check.cpp, which says what it checks).  No device; nothing is loaded into Python."""
from __future__ import annotations

import subprocess
from pathlib import Path

from arpeggia_amd import build as arp_build

ROOT = Path(__file__).resolve().parent.parent


def test_plan_and_carve_under_sanitizers(tmp_path):
    """Every block is a heap block of exactly its planned size, so an array that leaves it ends the program; so does pointer arithmetic on the null base of
    the planning walk."""
    prog = tmp_path / "carve_check"
    build = subprocess.run([arp_build.hipcc(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", str(ROOT / "tests" / "hostcheck" / "carve_check.cpp"), "-o", str(prog)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([str(prog)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout == "ok\n" and run.stderr == ""
