"""seq_compose_kernel (dexr_aux.hip) through dexr_seq_compose_dev on SYNTHETIC dof maps against the float64 loop of
tests/aux_reference.py (itself pinned to the reference project's recorded results in tests/test_aux_host.py).

Every value is random per (frame, sequence, dof), so a wrong row or sequence index shows; the maps mix target, fixed,
mimic-of-target and mimic-of-fixed dofs over permuted columns of rows wider than what is read.

Bound: 1e-12, the project's gate for this kernel.  Without the filter a target or fixed dof is a float32 -> float64
conversion times 1 plus 0, exact; a mimic dof is one multiply-add of |v| <= 4 (one rounding of a fused step against two:
<= 1e-15); a filtered frame adds one more such step, so nine frames stay below 1e-13.
"""
import numpy as np
import pytest

import aux_reference as ar
from dex_retargeting_amd import _lib

pytestmark = pytest.mark.gpu
TOL = 1e-12

# (B, n_q, T): B * n_q of 1, 255, 256 and 257 around the 256-thread block, several blocks, n_q = DEXR_MAX_DOF
SHAPES = [(1, 1, 1), (85, 3, 2), (64, 4, 2), (257, 1, 3), (67, 23, 9), (5, 64, 4)]
# (alpha, a filter buffer is passed, first_frame_initialises)
FILTERS = [(0.0, True, True), (0.0, True, False), (0.3, True, True), (0.3, True, False), (1.0, True, True),
           (1.0, True, False), (-1.0, False, True), (-1.0, True, False)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(require_gpu):
    yield


def dof_map(n_q, with_fixed, rng):
    """kind / idx / mult / off of n_q dofs: as many of the four sorts of dof as n_q allows, columns a non-identity
    permutation of rows three (two) wider than the target (fixed) dofs need, multipliers and offsets off 1 and 0."""
    sorts = ["target", "fixed", "mimic_fixed", "mimic_target"] if with_fixed else ["target", "mimic_target"]
    sort = [sorts[j % len(sorts)] for j in range(n_q)]
    if n_q > 4:
        sort = [sort[j] for j in rng.permutation(n_q)]
    tgt = [j for j in range(n_q) if sort[j] == "target"]
    fix = [j for j in range(n_q) if sort[j] == "fixed"]
    n_opt, n_fixed = len(tgt) + 3, (len(fix) + 2 if with_fixed else 0)
    kind, idx = np.zeros(n_q, np.int32), np.zeros(n_q, np.int32)
    mult, off = np.ones(n_q), np.zeros(n_q)
    for dofs, k, width in ((tgt, 0, n_opt), (fix, 1, n_fixed)):
        cols = rng.permutation(width)[: len(dofs)]
        while len(dofs) and np.array_equal(cols, np.arange(len(dofs))):
            cols = rng.permutation(width)[: len(dofs)]
        kind[dofs], idx[dofs] = k, cols
    for j in range(n_q):
        if sort[j].startswith("mimic"):
            src = fix if (sort[j] == "mimic_fixed" and fix) else tgt
            kind[j], idx[j] = 2, src[int(rng.integers(len(src)))]
            mult[j] = rng.choice([-1, 1]) * rng.uniform(0.5, 1.5)
            off[j] = rng.uniform(-0.5, 0.5)
    return kind, idx, mult, off, n_opt, n_fixed


class Guarded:
    """A float64 device array between two guard rows of NaN: the kernel gets the address of the middle."""

    def __init__(self, torch, shape, fill=None):
        self.t = torch.full((shape[0] + 2,) + tuple(shape[1:]), float("nan"), dtype=torch.float64, device="cuda")
        if fill is not None:
            self.t[1:-1].copy_(torch.from_numpy(fill))

    @property
    def ptr(self):
        return self.t[1].data_ptr()

    def read(self):
        a = self.t.cpu().numpy()
        assert np.all(np.isnan(a[0])) and np.all(np.isnan(a[-1])), "a guard row was written"
        return a[1:-1]


def run_kernel(torch, m, qraw, fixed, alpha, filt, first):
    """One dexr_seq_compose_dev call -> (out (T, B, n_q), filter state after the call or None)."""
    kind, idx, mult, off, n_opt, n_fixed = m
    T, B, n_q = qraw.shape[0], qraw.shape[1], len(kind)
    d_q = torch.from_numpy(qraw).cuda()
    d_f = torch.from_numpy(fixed).cuda() if fixed is not None else None
    out = Guarded(torch, (T, B * n_q))
    fl = Guarded(torch, (1, B * n_q), fill=filt.reshape(1, -1)) if filt is not None else None
    _lib.seq_compose_dev(B, T, kind, idx, mult, off, n_opt, n_fixed, d_q.data_ptr(), d_f.data_ptr() if d_f is not None else 0,
                         alpha, fl.ptr if fl is not None else 0, first, out.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.read().reshape(T, B, n_q), None if fl is None else fl.read().reshape(B, n_q)


worst = {"out": 0.0, "filt": 0.0}


@pytest.mark.parametrize("with_fixed", [True, False], ids=["mixed", "n_fixed_0"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-nq%d-T%d" % s)
def test_seq_compose_kernel_equals_the_float64_loop(shape, with_fixed):
    torch = pytest.importorskip("torch")
    B, n_q, T = shape
    rng = np.random.default_rng(B * 1000 + n_q * 10 + T + (0 if with_fixed else 7))
    m = dof_map(n_q, with_fixed, rng)
    kind, idx, mult, off, n_opt, n_fixed = m
    qraw = rng.uniform(-2, 2, (T, B, n_opt)).astype(np.float32)
    fixed = rng.uniform(-2, 2, (T, B, n_fixed)).astype(np.float32) if n_fixed else None  # n_fixed = 0: fixed is NULL
    plain = kind != 2
    for alpha, with_buffer, first in FILTERS:
        label = (shape, with_fixed, alpha, with_buffer, first)
        filt0 = rng.uniform(-3, 3, (B, n_q)) if with_buffer else None  # a carried state that is not zero
        want, want_filt = ar.seq_compose(kind, idx, mult, off, qraw, fixed, alpha, filt0, first)
        got, got_filt = run_kernel(torch, m, qraw, fixed, alpha, filt0, first)
        worst["out"] = max(worst["out"], float(np.abs(got - want).max()))
        assert np.abs(got - want).max() < TOL, label
        if alpha < 0:
            assert np.array_equal(got[:, :, plain], want[:, :, plain]), label  # conversions: exact
            if with_buffer:
                assert np.array_equal(got_filt, filt0), label                   # no filter: the buffer comes back untouched
            continue
        worst["filt"] = max(worst["filt"], float(np.abs(got_filt - want_filt).max()))
        assert np.abs(got_filt - want_filt).max() < TOL, label
        assert np.array_equal(got_filt, got[-1]), label  # the carried state is the last filtered row
        if first:
            assert np.array_equal(got[0][:, plain], want[0][:, plain]), label  # the first frame passes through: exact
        if T >= 2:  # one call over T1 + T2 frames == two calls that carry the filter, bit for bit
            T1 = T // 2
            a, fa = run_kernel(torch, m, qraw[:T1], None if fixed is None else fixed[:T1], alpha, filt0, first)
            b, fb = run_kernel(torch, m, qraw[T1:], None if fixed is None else fixed[T1:], alpha, fa, False)
            assert np.array_equal(np.concatenate([a, b]), got) and np.array_equal(fb, got_filt), label
    print(f"seq_compose {shape} with_fixed={with_fixed}: largest error so far out {worst['out']:.3e}, filter {worst['filt']:.3e}")
