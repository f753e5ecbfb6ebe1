"""The offline scoring's pair counts without a GPU: csrc/pair_counts.h compiled for the host and run in the
kernel's decomposition (csrc/pair_counts_host_check.cpp: a stand-alone program, built plain and under the address
and undefined-behaviour sanitizers) against numpy decode / OR / sum -- equal integers on every case of
pair_counts_cases.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pair_counts_cases as PC
from sam2_video.kernels import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sam2-video-training_amd", "csrc")


@pytest.fixture(scope="module")
def cases():
    cs = PC.make_cases()
    return cs, [PC.reference(c) for c in cs]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_check(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build csrc/pair_counts_host_check.cpp")
    exe = tmp_path_factory.mktemp("pair_counts_host") / f"pair_counts_host_check_{request.param}"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC,
                    os.path.join(CSRC, "pair_counts_host_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _side_bytes(groups, H, W):
    grp_off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    run_off, run_end = ops.rle_runs([c for g in groups for c in g], H, W)
    return grp_off.tobytes() + run_off.astype(np.int32).tobytes() + run_end.astype(np.int32).tobytes()


def run_host(exe, cases, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for c in cases:
            f.write(np.asarray([len(c["dt"]), c["H"], c["W"]], np.int32).tobytes())
            f.write(_side_bytes(c["dt"], c["H"], c["W"]))
            f.write(_side_bytes(c["gt"], c["H"], c["W"]))
    subprocess.run([exe, str(src), str(dst)], check=True, timeout=300)
    raw = np.frombuffer(dst.read_bytes(), np.uint64)
    out, off = [], 0
    for c in cases:
        n = 4 * len(c["dt"])
        out.append(raw[off:off + n].reshape(-1, 4).astype(np.int64))
        off += n
    assert off == raw.size
    return out


def test_the_cases_cover_what_they_claim(cases):
    cs, refs = cases
    assert {(c["H"], c["W"]) for c in cs} == set(PC.SIZES) and {len(c["dt"]) for c in cs} == {1, 37}
    assert 5 * 13 == 65  # one position into a second word
    by_name = {c["name"]: (c, r) for c, r in zip(cs, refs)}
    for H, W in PC.SIZES:
        c, r = by_name[f"{H}x{W}-G1-both_empty"]
        assert c["dt"] == [[]] and c["gt"] == [[]] and (r == 0).all()
        c, r = by_name[f"{H}x{W}-G1-empty_dt"]
        assert c["dt"] == [[]] and r[0, 2] == 0 and r[0, 0] == 0 and r[0, 1] == r[0, 3]
        c, r = by_name[f"{H}x{W}-G1-empty_gt"]
        assert c["gt"] == [[]] and r[0, 3] == 0 and r[0, 1] == r[0, 2]
        c, r = by_name[f"{H}x{W}-G1-full"]
        assert c["dt"] == [[[0, H * W]]] and r[0, 2] == H * W == r[0, 1]
        c, r = by_name[f"{H}x{W}-G1-single_run"]
        assert c["dt"] == [[[H * W]]] and r[0, 2] == 0
        c, r = by_name[f"{H}x{W}-G1-zero_first_run"]
        assert c["dt"][0][0][0] == 0 and r[0, 2] > 0
        c, r = by_name[f"{H}x{W}-G1-three_overlapping"]
        assert 3 in (len(c["dt"][0]), len(c["gt"][0]))
    assert any(r[:, 0].max() > 0 for r in refs)  # the sides do overlap somewhere


def test_header_counts_equal_numpy(host_check, cases, tmp_path):
    cs, refs = cases
    got = run_host(host_check, cs, tmp_path)
    for c, g, want in zip(cs, got, refs):
        assert g.shape == want.shape and (g == want).all(), (c["name"], g[(g != want).any(axis=1)][:3])


def test_host_check_refuses_bad_sizes(host_check, tmp_path):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(np.asarray([1, 0, 4], np.int32).tobytes())
    assert subprocess.run([host_check, str(src), str(dst)], timeout=60).returncode == 3
