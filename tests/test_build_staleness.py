"""accel_rl_amd/_build.py's staleness rule on a throw-away tree: a library is current until a source or a public header
changes, whatever the build writes next to its objects (csrc/_obj) afterwards.  A library that read as stale right after
its own build made every later build() -- bench.py's, a test run's -- rebuild, which fails where the tree is read-only."""
import os
import time

import pytest

from accel_rl_amd import _build


@pytest.fixture
def tree(tmp_path, monkeypatch):
    root = tmp_path / "repo"
    csrc = root / "accel_rl_amd" / "csrc"
    (csrc / "_obj").mkdir(parents=True)
    (root / "include").mkdir()
    for f in ("a.hip", "b_dev.h"):
        (csrc / f).write_text("// source\n")
    for h in ("accel_rl_hip.h", "accel_rl_hip_dev.h"):
        (root / "include" / h).write_text("// header\n")
    lib = root / "accel_rl_amd" / "libaccel_rl_hip.so"
    monkeypatch.setattr(_build, "ROOT", str(root))
    monkeypatch.setattr(_build, "CSRC", str(csrc))
    monkeypatch.setattr(_build, "LIB_PATH", str(lib))
    monkeypatch.delenv("ARL_HIPCC_FLAGS", raising=False)
    return root, csrc, lib


def _later(path, t0):
    """give `path` a modification time after t0 (the file system's clock may be coarse)"""
    os.utime(path, (t0 + 5, t0 + 5))


def test_library_is_current_after_its_build_wrote_the_flags_stamp(tree):
    root, csrc, lib = tree
    assert _build._stale()                                   # no library yet
    lib.write_bytes(b"\x7fELF")
    t0 = os.path.getmtime(lib)
    for p in [csrc / "a.hip", csrc / "b_dev.h", root / "include" / "accel_rl_hip.h",
              root / "include" / "accel_rl_hip_dev.h"]:
        os.utime(p, (t0 - 10, t0 - 10))
    stamp = csrc / "_obj" / ".flags"
    stamp.write_text("hipcc ...||")                          # written after the link, as _build_locked does
    (csrc / "_obj" / "a.o").write_bytes(b"")
    _later(stamp, t0)
    _later(csrc / "_obj", t0)                                # the directory's time moved past the library's
    assert not _build._stale()


@pytest.mark.parametrize("dep", ["accel_rl_amd/csrc/a.hip", "accel_rl_amd/csrc/b_dev.h", "include/accel_rl_hip.h",
                                 "include/accel_rl_hip_dev.h"])
def test_a_changed_source_or_header_makes_it_stale(tree, dep):
    root, csrc, lib = tree
    lib.write_bytes(b"\x7fELF")
    t0 = time.time() - 100
    for p in [csrc / "a.hip", csrc / "b_dev.h", root / "include" / "accel_rl_hip.h",
              root / "include" / "accel_rl_hip_dev.h"]:
        os.utime(p, (t0, t0))
    os.utime(lib, (t0 + 1, t0 + 1))
    assert not _build._stale()
    _later(root / dep, t0 + 1)
    assert _build._stale()


def test_other_flags_make_it_stale(tree, monkeypatch):
    root, csrc, lib = tree
    lib.write_bytes(b"\x7fELF")
    (csrc / "_obj" / ".flags").write_text("hipcc ...||")
    t0 = os.path.getmtime(lib)
    for p in [csrc / "a.hip", csrc / "b_dev.h", root / "include" / "accel_rl_hip.h",
              root / "include" / "accel_rl_hip_dev.h"]:
        os.utime(p, (t0 - 10, t0 - 10))
    assert not _build._stale()
    monkeypatch.setenv("ARL_HIPCC_FLAGS", "-DARL_NO_SPLIT6")
    assert _build._stale()
