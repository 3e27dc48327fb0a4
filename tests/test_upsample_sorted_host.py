"""The test that lets k_upsample (csrc/volsdf_render.hip) leave out its sort - csrc/sample_cdf.h::lane_row_in_order over the row that invert_cdf_at
wrote - as host code: tests/upsample_sorted_host.cpp includes the header the kernel includes, builds rows the way the kernel does and prints, per
row, what a plain scan says (truth) and what the 64 lanes' test says (verdict).  A row that is out of order, or holds a NaN, must never pass: that
is the only way the shortcut could change a bit.  No GPU; the program is built with the address and undefined-behaviour sanitizers where the host
compiler has them and run directly."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "upsample_sorted_host.cpp")
CSRC = os.path.join(ROOT, "nerfart_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("upsorted") / "upsample_sorted_host")
    base = [CXX, "-std=c++17", "-O1", "-g", "-I", CSRC, SRC, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:                                    # a compiler without the sanitizer runtimes: the plain program checks the same verdicts
        r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    out = {}
    for line in run.stdout.splitlines():
        m = re.match(r"(\S+) n=(\d+) truth=(\w+) verdict=(\w+)$", line)
        assert m, line
        out[m.group(1)] = (int(m.group(2)), m.group(3), m.group(4))
    return out


def test_the_kernel_and_the_program_share_the_code():
    text = open(os.path.join(CSRC, "volsdf_render.hip")).read()
    assert "lane_row_in_order(out, P.n_up, lane)" in text
    assert '#include "sample_cdf.h"' in open(os.path.join(CSRC, "ray_common.h")).read()
    hdr = open(os.path.join(CSRC, "sample_cdf.h")).read()
    assert "invert_cdf_at" in hdr and "lane_row_in_order" in hdr


@pytest.mark.parametrize("family", ["equal_run", "one_ulp_bin", "u_on_cdf_entry"])
def test_rows_built_to_break_the_order_are_reported(rows, family):
    mine = {k: v for k, v in rows.items() if k.startswith(family)}
    assert len(mine) == 5, sorted(rows)                      # inside a lane's stride, across lane 63 -> 0, at the row's end
    for name, (n, truth, verdict) in mine.items():
        assert n == 512
        assert truth == "unsorted", f"{name}: the row was meant to be out of order"
        assert verdict == "unsorted", f"{name}: a row that is out of order passed the lane test"


def test_nan_rows_are_reported(rows):
    for name in ("nan_one_bin", "nan_last_element", "nan_everywhere"):
        assert rows[name][1:] == ("unsorted", "unsorted"), (name, rows[name])


def test_minus_zero_next_to_zero_is_reported(rows):
    """ascending as numbers, but a sort may move the -0 (its descending stages exchange equal elements): the lane test must not pass it"""
    assert rows["minus_zero_among_zeros"][1:] == ("sorted", "unsorted")


def test_smooth_rows_are_in_order(rows):
    mine = {k: v for k, v in rows.items() if k.startswith("smooth_")}
    assert len(mine) == 9
    for name, (n, truth, verdict) in mine.items():
        assert (n, truth, verdict) == (512, "sorted", "sorted"), (name, n, truth, verdict)


def test_no_row_that_is_out_of_order_passes(rows):
    assert len(rows) >= 28
    for name, (_, truth, verdict) in rows.items():
        assert not (truth == "unsorted" and verdict == "sorted"), name
