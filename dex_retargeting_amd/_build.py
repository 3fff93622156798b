"""Build libdexr.so (hipcc, gfx950) in-tree.  Used by __graft_entry__.build(); hipcc cross-compiles without a GPU."""
from __future__ import annotations

import functools
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(REPO, "include")
BUILD = os.environ.get("DEXR_BUILD_DIR") or os.path.join(REPO, "build")
LIB = os.environ.get("DEXR_LIB_OUT") or os.path.join(HERE, "libdexr.so")
BUCKETS = (4, 8, 16, 24, 32)
CHAIN_BUCKETS = (4,)
VARIANTS = ((0, 0), (1, 0), (1, 1), (1, 2))  # (float64?, mode): f32 solve, f64 solve, f64 eval, f64 fk
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{INCLUDE}", f"-I{CSRC}"] + \
    os.environ.get("DEXR_EXTRA_FLAGS", "").split()
# The SLP vectoriser turns the 3-vector arithmetic of the register kernels into v_pk_* pairs that it then has to
# assemble with v_mov_b32 (342 moves in the 4-joint chain kernel) and that need aligned register pairs: without it the
# same kernel has 9 % fewer VALU instructions, 126 instead of 156 VGPRs (4 waves per SIMD, no scratch) and runs
# 25 % faster (Allegro vector 0.108 -> 0.081 ms per 65 536 frames; Shadow vector 9.4 -> 4.3 ms).
# float32 divisions / square roots of the solver (step scaling, Huber weights, Cholesky pivots) do not need IEEE
# rounding or denormal support -- parity is measured against the float64 oracle: 2.5-ulp v_rcp/v_rsq sequences and
# flushed denormals save another 8 % of the chain kernel's VALU instructions.
NO_SLP = ["-fno-slp-vectorize", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-fgpu-flush-denormals-to-zero"]


def _inst(n: int, f64: int, *defs: str) -> list:
    """Flags of a solve-mode (DEXR_MODE=0) instantiation of dexr_inst.hip."""
    return NO_SLP + [f"-DDEXR_NMAX={n}", f"-DDEXR_F64={f64}", "-DDEXR_MODE=0", *defs]


_INST, _WIDE = "dexr_inst.hip", "dexr_wide_inst.hip"
_MIMIC, _MODCHOL, _SPRINT = "-DDEXR_MIMIC=1", "-DDEXR_MODCHOL=1", "-DDEXR_SPRINT=1"
# Everything libdexr.so is made of, in link order: (object file, source file, flags after FLAGS).  Host-side units first;
# dexr_pose is the link poses + their VJP (include/dexr_pose.h), the link Jacobians / velocities (include/dexr_jacobian.h) and
# the link wrenches / velocity VJP (include/dexr_wrench.h): a unit of its own, in no workload's source hash.
OBJECTS = [(f"dexr_{u}.o", f"dexr_{u}.hip", []) for u in ("api", "prep", "aux", "comm", "pose")]
OBJECTS += [("dexr_gen.o", "dexr_gen_inst.hip", [])]
# register kernel of small components, biggest first so the thread pool stays busy (jobs start in table order);
# bucket 32 serves float32 requests with its float64 kernel (see dexr_launch.hpp)
OBJECTS += [(f"dexr_inst_{n}_{f64}_{mode}.o", _INST, NO_SLP + [f"-DDEXR_NMAX={n}", f"-DDEXR_F64={f64}", f"-DDEXR_MODE={mode}"])
            for n in sorted(BUCKETS, reverse=True) for f64, mode in VARIANTS if (n, f64, mode) != (32, 0, 0)]
# sixteen-lanes-per-frame kernel for dense components
# (the 16-row grid fits three waves per SIMD: 168 VGPRs, 18 of them spilled; 11.8 KB of LDS per wave)
OBJECTS += [(f"dexr_wide_{n}.o", _WIDE, NO_SLP + [f"-DDEXR_NMAX={n}"] + (["-DDEXR_WIDE_MINW=3"] if n == 16 else []))
            for n in (16, 24, 32)]
# ... one frame per wave (SPRINT): the launch shape of small batches
# (register budgets: two waves per SIMD for the 16- / 24-row grids (246 / 256 registers, 3 spilled at n = 24), one for
# the 32-row grid (272): small batches do not need the occupancy)
OBJECTS += [(f"dexr_wide_s_{n}.o", _WIDE, NO_SLP + [f"-DDEXR_NMAX={n}", _SPRINT, "-DDEXR_WIDE_MINW=1" if n == 32 else "-DDEXR_WIDE_MINW=2"])
            for n in (16, 24, 32)]
# the same kernel on the grid of the optimised variables (mimic joints): one frame per wave, then sixteen lanes per frame;
# plain / modified Cholesky each
OBJECTS += [(f"dexr_wide_{tag}_16.o", _WIDE, NO_SLP + ["-DDEXR_NMAX=16", _MIMIC] + defs)
            for tag, defs in (("s_m", [_SPRINT]), ("s_mc", [_SPRINT, _MODCHOL]), ("m", []), ("mc", [_MODCHOL]))]
# ... its float64 instantiation (dexr_tuning.kernel_f64): one wave per SIMD, four frames per wave
OBJECTS += [(f"dexr_wide_d_{tag}.o", _WIDE, NO_SLP + defs + ["-DDEXR_WIDE_F64=1"])
            for tag, defs in (("16", ["-DDEXR_NMAX=16"]), ("24", ["-DDEXR_NMAX=24"]), ("m_16", ["-DDEXR_NMAX=16", _MIMIC]),
                              ("mc_16", ["-DDEXR_NMAX=16", _MIMIC, _MODCHOL]))]
# reduced-variable kernel (mimic models): Hessian of the variables in registers
OBJECTS += [(f"dexr_red_{nv}.o", "dexr_red_inst.hip", NO_SLP + [f"-DDEXR_NV={nv}"]) for nv in (8, 16)]
# small components with fleet / sequence addressing (EXT)
OBJECTS += [(f"dexr_inst_ext_{n}_{f64}_0.o", _INST, _inst(n, f64, "-DDEXR_EXT=1")) for n, f64 in ((4, 0), (8, 0), (4, 1), (8, 1))]
OBJECTS += [(f"dexr_inst_ext_chain_{n}_0_0.o", _INST, _inst(n, 0, "-DDEXR_CHAIN=1", "-DDEXR_EXT=1")) for n in CHAIN_BUCKETS]
# tip pass of the serial-chain kernel (dexr_tip.hpp): float32, and float64 (the reference's arithmetic)
OBJECTS += [(f"dexr_inst_{tag}_4_{f64}_0.o", _INST, _inst(4, f64, "-DDEXR_CHAIN=1", "-DDEXR_TIP=1", *defs))
            for f64 in (0, 1) for tag, defs in (("tip", []), ("ext_tip", ["-DDEXR_EXT=1"]))]
# the float32 tip solve as a kernel of its own (dexr_tip_solve.hpp): plain tile launches
OBJECTS += [("dexr_tip32.o", "dexr_tip_inst.hip", NO_SLP)]
# serial-chain specialisation, float32 solve only
OBJECTS += [(f"dexr_inst_chain_{n}_0_0.o", _INST, _inst(n, 0, "-DDEXR_CHAIN=1")) for n in CHAIN_BUCKETS]


# Which sources decide the code a bench workload's dominant kernel runs (used to key the committed rocprofv3 PMC
# summaries, profiles/pmc_<workload>.json: bench.py attaches their counters to a line only while this hash is unchanged).
_COMMON_SOURCES = ["dexr_api.hip", "dexr_launch.hpp", "../../include/dexr.h", "../../include/dexr_tables.h"]
KERNEL_SOURCES = {
    "allegro_vector": ["dexr_kernel.hpp", "dexr_tip.hpp", "dexr_tip_solve.hpp", "dexr_tip_inst.hip", "dexr_math.hpp", "dexr_inst.hip"],
    "shadow_dexpilot": ["dexr_wide.hpp", "dexr_wide_inst.hip", "dexr_math.hpp"],
    "leap_position": ["dexr_wide.hpp", "dexr_wide_inst.hip", "dexr_math.hpp"],
    # sub-records of the default line (bench.py --probe): the float64 / cold-start launches of the headline config, the general
    # kernel; "mixed_fleet" is absent on purpose: four robots = every kernel family, i.e. all sources (the fallback)
    "allegro_vector_f64": ["dexr_kernel.hpp", "dexr_tip.hpp", "dexr_math.hpp", "dexr_inst.hip"],
    "allegro_vector_cold": ["dexr_kernel.hpp", "dexr_tip.hpp", "dexr_tip_solve.hpp", "dexr_tip_inst.hip", "dexr_math.hpp", "dexr_inst.hip"],
    "general_kernel": ["dexr_gen.hpp", "dexr_gen_inst.hip", "dexr_kernel.hpp", "dexr_math.hpp"],
}


def source_hash(workload: str) -> str:
    """sha256[:16] over the sources (names + contents) and compiler flags that produce `workload`'s dominant kernel."""
    import hashlib

    names = sorted(set(KERNEL_SOURCES.get(workload) or [f for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))]) | set(_COMMON_SOURCES))
    h = hashlib.sha256()
    for n in names:
        h.update(os.path.basename(n).encode())
        with open(os.path.normpath(os.path.join(CSRC, n)), "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS[:4] + NO_SLP).encode())
    return h.hexdigest()[:16]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


@functools.lru_cache(maxsize=None)
def _includes(path: str) -> tuple:
    """The files `path` names in `#include "..."` lines, each found in csrc/ or include/ (one scan per file)."""
    with open(path) as f:
        names = _INCLUDE.findall(f.read())
    found = []
    for n in names:
        hits = [p for p in (os.path.join(CSRC, n), os.path.join(INCLUDE, n)) if os.path.exists(p)]
        if not hits:
            raise RuntimeError(f"{path} includes {n!r}, which is in neither csrc/ nor include/")
        found.append(hits[0])
    return tuple(found)


def _deps(source: str) -> set:
    """`source` and the transitive closure of its quoted includes: what an object compiled from it depends on."""
    todo, seen = [source], set()
    while todo:
        p = todo.pop()
        if p not in seen:
            seen.add(p)
            todo += _includes(p)
    return seen


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _pool_limit() -> int:
    """Compile jobs to run at once: MAX_JOBS or CMAKE_BUILD_PARALLEL_LEVEL (the first set to a positive integer), never
    more than 16 or than this machine's CPUs.  Not os.cpu_count() alone: a shared machine reports CPUs a build may not use."""
    asked = [int(v) for v in (os.environ.get(k, "").strip() for k in ("MAX_JOBS", "CMAKE_BUILD_PARALLEL_LEVEL")) if v.isdigit() and int(v) > 0]
    return min(asked[0] if asked else 16, 16, os.cpu_count() or 16)


def build_library(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(BUILD, exist_ok=True)
    hipcc = _hipcc()
    # developer shortcut: DEXR_BUILD_ONLY="4,8" rebuilds only those buckets and reuses the other buckets' objects as they are
    # (only valid while KernelParams / the launcher signature are unchanged)
    only = os.environ.get("DEXR_BUILD_ONLY")
    reuse = set() if not only else {f"dexr_inst_{n}_{f64}_{mode}.o" for n in set(BUCKETS) - {int(v) for v in only.split(",")}
                                    for f64, mode in VARIANTS}
    jobs = []
    objs = []
    for name, source, flags in OBJECTS:
        s, o = os.path.join(CSRC, source), os.path.join(BUILD, name)
        objs.append(o)
        if name in reuse and os.path.exists(o):
            continue
        if force or _stale(o, _deps(s)):
            jobs.append((s, o, flags))

    def compile_one(job):
        s, o, defs = job
        cmd = [hipcc] + FLAGS + defs + ["-c", s, "-o", o]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {s}:\n{r.stderr[-4000:]}")
        if verbose:
            print("compiled", os.path.basename(o), file=sys.stderr)
        return o

    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), _pool_limit())) as ex:
            list(ex.map(compile_one, jobs))
    if force or jobs or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr[-4000:]}")
    return LIB


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
