"""The host-only pieces of klsh_save_clusters under AddressSanitizer + UndefinedBehaviorSanitizer
(CPU only): `make -C kmerlsh_amd/csrc save_plan` builds tests/cpp/save_plan_main.cpp over
kmerlsh_amd/csrc/klsh_save_plan.h — the path probe that refuses a call before a file is touched,
the chunk rule, the tiles of a text window and the clipping arithmetic the emit kernel shares,
replayed store by store into buffers of exactly a window's bytes.  Any report aborts: exit 0 =
clean.
"""
import os
import subprocess

import pytest

from conftest import ROOT

DRIVER = os.path.join(ROOT, "kmerlsh_amd", "build_asan", "save_plan_main")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def driver():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "kmerlsh_amd", "csrc"), "save_plan"],
                   check=True, capture_output=True, timeout=600)
    return DRIVER


def run(args):
    p = subprocess.run(args, env=ENV, capture_output=True, text=True, timeout=300)
    report = "AddressSanitizer" in p.stderr or "runtime error" in p.stderr or "LeakSanitizer" in p.stderr
    assert p.returncode == 0 and not report, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def test_path_probe_sanitized(driver, tmp_path):
    assert "paths ok" in run([driver, "paths", str(tmp_path)])
    assert os.listdir(tmp_path) == []


def test_chunk_windows_sanitized(driver):
    assert "windows ok" in run([driver, "windows"])
