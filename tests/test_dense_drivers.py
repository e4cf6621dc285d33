"""The dense drivers of the narrow hour (csrc/cpm_narrow.h, "dense drivers") on the CPU: tests/dense_probe.cc compiles the product's
own index arithmetic -- a driver's rank from its slot's ballot, the scratch's capacity, the dense slots read back and which of their
lanes are live -- for the host and holds it against a plain loop for every ballot pattern class; and the rule that says which twin
<CPT, rung> compacts is held against the blocks a CU's LDS keeps, restated here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("dense") / "dense_probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "dense_probe.cc")], check=True)
    return exe


def test_compaction_against_a_plain_loop(probe):
    r = subprocess.run([probe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 30000, r.stdout


CU_LDS, STEP, STATIC, LIST = 160 * 1024, 1280, 4240, 10240   # a CU's LDS, its assumed allocation step, a block's static bytes, the placing list
BY_REGISTERS = {1: 7, 2: 7, 4: 7, 6: 6}                        # blocks per CU the twin's registers allow (the resource remarks)


def test_compaction_is_on_only_where_the_cu_keeps_its_blocks(probe):
    """per cell of the hour's ladder: with the scratch behind the largest narrow pack of the rung's band, a CU still holds the blocks
    the uncompacted twin runs there; the headline's cell <6, 5> compacts and the cells above Z = 4,096 at four and six cars do not"""
    r = subprocess.run([probe, "fits"], capture_output=True, text=True, check=True)
    cells = {}
    for line in r.stdout.splitlines():
        f = line.split()
        assert f[0] == "F"
        cpt, rung, top, pack, pays, fits, on, scratch = map(int, f[1:])
        cells[cpt, rung] = on
        assert on == (pays and fits) and scratch == (4 * 64 * cpt * 8 if on else 0), line
        before = max(pack, LIST) + STATIC
        after = max(pack + 4 * 64 * cpt * 8, LIST) + STATIC
        kept = min(BY_REGISTERS[cpt], CU_LDS // before)
        if on:
            assert -(-after // STEP) * STEP * kept <= CU_LDS, line
        if pays and not fits:
            assert after * kept > CU_LDS - STEP * kept, line   # (switched off for a reason: at most the rounding away from fitting)
    assert len(cells) == 32
    assert cells[6, 5] and cells[4, 5] and cells[1, 5] and not cells[2, 5]
    assert not cells[6, 6] and not cells[4, 6] and not cells[6, 12] and not cells[4, 12]
