"""CPU: what _build.build_library compiles and links, what each object depends on, and how many compilers run at once.

tests/golden/build_plan.json is the plan of the commit before the OBJECTS table: per object, in link order, [object, source,
flags after FLAGS], and the link command after the compiler's name, paths reduced to basenames.  It was recorded from that
commit's build_library, not from the table; to record it again, run in a checkout of the commit to compare against, with
DEXR_EXTRA_FLAGS unset and DEXR_BUILD_DIR / DEXR_LIB_OUT pointing into an empty directory:

    import json, os, subprocess, sys, types
    from dex_retargeting_amd import _build as b
    cmds = []
    subprocess.run = lambda cmd, **kw: cmds.append(cmd) or types.SimpleNamespace(returncode=0, stderr="")
    b.build_library(force=True)
    base, n = os.path.basename, 1 + len(b.FLAGS)
    rows = [json.dumps([base(c[-1]), base(c[-3]), c[n:-4]]) for c in cmds[:-1]]  # that commit compiles in link order
    link = json.dumps([base(a) for a in cmds[-1][1:]])
    open(sys.argv[1], "w").write('{"objects": [\\n' + ",\\n".join(rows) + '],\\n"link": ' + link + "}\\n")
"""
import json
import os
import shutil
import subprocess
import types

import pytest

from testutil import REPO
from dex_retargeting_amd import _build

SOURCES = sorted({src for _, src, _ in _build.OBJECTS})


class _Recorder:
    """Stands in for subprocess.run and ThreadPoolExecutor inside _build: nothing is compiled, everything is noted."""

    def __init__(self, monkeypatch, build_dir):
        self.cmds, self.workers = [], []
        monkeypatch.setattr(_build, "BUILD", str(build_dir))
        monkeypatch.setattr(_build, "LIB", str(build_dir / "libdexr.so"))
        monkeypatch.setattr(_build, "subprocess", types.SimpleNamespace(run=self._run))
        monkeypatch.setattr(_build, "ThreadPoolExecutor", self._pool)

    def _run(self, cmd, **kw):
        self.cmds.append(list(cmd))
        return types.SimpleNamespace(returncode=0, stderr="")

    def _pool(self, max_workers):
        self.workers.append(max_workers)
        return _SerialPool()

    def compiled(self):
        """{object basename: (source basename, flags after FLAGS)} of the recorded compile commands."""
        n = 1 + len(_build.FLAGS)
        out = {}
        for c in self.cmds:
            if "-c" in c:
                assert c[1:n] == _build.FLAGS and c[-4] == "-c" and c[-2] == "-o", c
                out[os.path.basename(c[-1])] = (os.path.basename(c[-3]), c[n:-4])
        return out

    def links(self):
        return [[os.path.basename(a) for a in c[1:]] for c in self.cmds if "-shared" in c]


class _SerialPool:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def map(self, fn, jobs):
        return [fn(j) for j in jobs]


def test_plan_is_what_the_parent_commit_built(monkeypatch, tmp_path):
    with open(os.path.join(REPO, "tests", "golden", "build_plan.json")) as f:
        want = json.load(f)
    assert len(want["objects"]) == 52
    rec = _Recorder(monkeypatch, tmp_path)
    _build.build_library(force=True)
    (link,) = rec.links()
    assert link == want["link"]
    compiled = rec.compiled()
    assert len(compiled) == len(rec.cmds) - 1 == 52, "one compile per object, one link"
    got = [[o, compiled[o][0], compiled[o][1]] for o in link if o.endswith(".o")]
    assert got == want["objects"]
    assert [[o, s, f] for o, s, f in _build.OBJECTS] == want["objects"], "the table itself reads as the plan"


@pytest.mark.parametrize("source", SOURCES)
def test_include_scan_matches_the_compiler(source):
    path = os.path.join(_build.CSRC, source)
    # (with the flags of the first object built from it: dexr_inst.hip and its like refuse to compile without their -D)
    flags = next(f for _, s, f in _build.OBJECTS if s == source)
    r = subprocess.run([_build._hipcc()] + _build.FLAGS + flags + ["-M", "--cuda-host-only", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    reported = [os.path.realpath(t) for t in r.stdout.replace("\\\n", " ").split()[1:]]  # after "<object>:"
    root = os.path.realpath(REPO) + os.sep
    want = {os.path.basename(p) for p in reported if p.startswith(root)}
    got = {os.path.basename(p) for p in _build._deps(path)}
    assert source in got and got == want, (sorted(got ^ want), source)


@pytest.fixture
def up_to_date_tree(monkeypatch, tmp_path):
    """A copy of the sources whose every object exists and is newer than they are; yields (recorder, csrc, include)."""
    csrc, include, build = tmp_path / "csrc", tmp_path / "include", tmp_path / "build"
    shutil.copytree(_build.CSRC, csrc)
    shutil.copytree(_build.INCLUDE, include)
    monkeypatch.setattr(_build, "CSRC", str(csrc))
    monkeypatch.setattr(_build, "INCLUDE", str(include))
    build.mkdir()
    rec = _Recorder(monkeypatch, build)
    newest = max(os.path.getmtime(os.path.join(d, f)) for d in (csrc, include) for f in os.listdir(d))
    for name in [o for o, _, _ in _build.OBJECTS] + ["libdexr.so"]:
        (build / name).write_bytes(b"")
        os.utime(build / name, (newest + 10, newest + 10))
    _build.build_library()
    assert rec.cmds == [], "nothing is stale yet"
    return rec, csrc, include


def _touch_after_objects(path):
    t = os.path.getmtime(path) + 100  # the objects are 10 s newer than the newest source
    os.utime(path, (t, t))


def test_a_newer_wide_header_requeues_the_wide_objects_only(up_to_date_tree):
    rec, csrc, _ = up_to_date_tree
    _touch_after_objects(csrc / "dexr_wide.hpp")
    _build.build_library()
    wide = {o for o, s, _ in _build.OBJECTS if s == "dexr_wide_inst.hip"}
    f64 = {o for o, _, flags in _build.OBJECTS if "-DDEXR_WIDE_F64=1" in flags}
    assert f64 == {f"dexr_wide_d_{t}.o" for t in ("16", "24", "m_16", "mc_16")} and f64 < wide and len(wide - f64) == 10
    assert all(o.startswith("dexr_wide") for o in wide)
    assert set(rec.compiled()) == wide
    assert len(rec.links()) == 1


def test_a_newer_math_header_requeues_pose_and_every_kernel_object(up_to_date_tree):
    rec, csrc, _ = up_to_date_tree
    _touch_after_objects(csrc / "dexr_math.hpp")
    _build.build_library()
    # (dexr_api.o too: it instantiates the launchers, dexr_launch.hpp -> dexr_kernel.hpp -> dexr_tip.hpp -> dexr_math.hpp)
    assert set(rec.compiled()) == {o for o, _, _ in _build.OBJECTS} - {"dexr_prep.o", "dexr_aux.o", "dexr_comm.o"}


@pytest.mark.parametrize("env,workers", [({}, 16), ({"MAX_JOBS": "4"}, 4), ({"MAX_JOBS": "64"}, 16),
                                         ({"CMAKE_BUILD_PARALLEL_LEVEL": "4"}, 4), ({"MAX_JOBS": "0", "CMAKE_BUILD_PARALLEL_LEVEL": "6"}, 6)])
def test_pool_size_ignores_the_cpu_count_of_a_big_machine(monkeypatch, tmp_path, env, workers):
    for k in ("MAX_JOBS", "CMAKE_BUILD_PARALLEL_LEVEL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(os, "cpu_count", lambda: 384)
    rec = _Recorder(monkeypatch, tmp_path)
    _build.build_library(force=True)
    assert len(rec.compiled()) == 52
    assert rec.workers == [workers]
