"""The closed-form fit of gmp (opendpd_amd/fit.py, csrc/gmp_ls.hip), the parts that need no GPU: the comparator every test of the
feature measures against (a numpy fp64 restatement of the reference's gmp basis, pinned on the reference's recorded output), the host
solve, and the two new C ABI calls' declarations, size query and refusals."""
import ctypes as C
import functools
import os
import re

import numpy as np

from tests.golden_util import GOLDEN, Fixture, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
M, NP, P = 11, 4, 495


# ---- the comparator (not the code under test) -----------------------------------------------------------------------------------------
def basis(x):
    """(T, 2) I/Q samples -> complex (T, 495): the terms Weight[0, :] multiplies (backbones/gmp.py:25-46), zero history, in fp64"""
    x = np.asarray(x, dtype=np.float64)
    T = len(x)
    u = np.concatenate([np.zeros(M - 1, dtype=np.complex128), x[:, 0] + 1j * x[:, 1]])           # gmp.py:26-27
    a = np.concatenate([np.zeros(2 * (M - 1)), np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])])  # gmp.py:33
    pw = [a, a * a, a * a * a, (a * a) * (a * a)]
    t = np.arange(T)
    cols = [u[t + m] for m in range(M)]                                                           # x_input (gmp.py:43)
    cols += [u[t + m] * pw[d][t + i + m] for d in range(NP) for i in range(M) for m in range(M)]  # mul_term, (d, i, m) (gmp.py:44-45)
    return np.stack(cols, axis=1)


def design(x, target):
    """the real design matrix [A | b] of sequences (B, T, 2): per sequence the rows of the real parts, then of the imaginary parts"""
    rows = []
    for xs, ts in zip(np.asarray(x), np.asarray(target, dtype=np.float64)):
        phi = basis(xs)
        rows.append(np.concatenate([np.concatenate([phi.real, ts[:, :1]], 1), np.concatenate([phi.imag, ts[:, 1:]], 1)], 0))
    return np.concatenate(rows, 0)


def gram(x, target):
    A = design(x, target)
    return A.T @ A


@functools.lru_cache(maxsize=None)
def dataset():
    d = np.load(os.path.join(GOLDEN, "dpa200_dataset.npz"))
    return {k: d[k].astype(np.float32) for k in d.files if k != "spec"}      # the samples as the kernels see them: fp32


@functools.lru_cache(maxsize=None)
def train_design():
    """[A | b] of the dataset's training stream as one sequence, and its Gram matrix (computed once per session, never written to)"""
    d = dataset()
    A = design(d["train_input"][None], d["train_output"][None])
    G = A.T @ A
    A.setflags(write=False); G.setflags(write=False)
    return A, G


def reference_solution(G, ridge):
    """(w, e_max) of the comparator: numpy.linalg.solve on the regularised normal equations"""
    N, r = G[:P, :P], G[:P, P]
    e_max = float(np.linalg.eigvalsh(N)[-1])
    return np.linalg.solve(N + ridge * e_max * np.eye(P), r), e_max


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
def test_the_comparator_reproduces_the_reference_output():
    fx = Fixture("gmp_m11")
    w = fx["sd/backbone.Weight"].astype(np.float64).reshape(-1)
    for xk, yk in (("x", "y"), ("xa", "ya")):
        got = np.stack([basis(xs) @ w for xs in fx[xk]])
        ref = fx[yk][..., 0] + 1j * fx[yk][..., 1]
        assert rel_err(np.stack([got.real, got.imag], -1), np.stack([ref.real, ref.imag], -1)) < 1e-5, xk


def test_solve_ridge_equals_a_direct_solve_of_the_regularised_system():
    from opendpd_amd.fit import solve_ridge
    A, G = train_design()
    for ridge in (1e-8, 1e-6):
        sol = solve_ridge(G, ridge)
        w_ref, e_max = reference_solution(G, ridge)
        assert sol.w.shape == (P,) and sol.w.dtype == np.float64
        assert abs(sol.e_max - e_max) <= 1e-12 * e_max and sol.e_min < 1e-9 * sol.e_max      # numerically singular
        pred, pred_ref = A[:, :P] @ sol.w, A[:, :P] @ w_ref
        err = np.max(np.abs(pred - pred_ref)) / np.max(np.abs(pred_ref))
        print(f"ridge {ridge:g}: max|w| {np.max(np.abs(sol.w)):.3f}, prediction error {err:.3g}")
        assert err < 1e-9, (ridge, err)
        direct = float(np.sum((pred - A[:, P]) ** 2))
        assert abs(sol.residual - direct) < 1e-9 * direct, (ridge, sol.residual, direct)


def test_solve_ridge_of_a_rank_deficient_sequence_is_finite():
    from opendpd_amd.fit import solve_ridge
    x = np.tile(np.array([[0.3, -0.4]], dtype=np.float32), (64, 1))[None]
    G = gram(x, 2.0 * x)
    sol = solve_ridge(G)
    assert np.linalg.matrix_rank(G[:P, :P]) < P
    assert np.all(np.isfinite(sol.w)) and np.isfinite(sol.residual) and sol.e_max > 0
    # a sequence of zeros: nothing to fit, no weight
    zero = solve_ridge(np.zeros((P + 1, P + 1)))
    assert np.all(zero.w == 0) and zero.residual == 0


def _lib_and_desc():
    import __graft_entry__ as g
    g.build()
    from opendpd_amd import _lib
    return _lib, _lib.load()


def test_the_new_symbols_are_declared_exported_and_bound():
    _lib, lib = _lib_and_desc()
    header = open(os.path.join(ROOT, "include", "opendpd_hip.h")).read()
    declared = set(re.findall(r"\b(odpd_[a-z_0-9]+)\s*\(", header))
    for sym in ("odpd_gmp_gram_workspace_bytes", "odpd_gmp_gram"):
        assert sym in declared and sym in _lib.exported_symbols() and hasattr(lib, sym), sym
    assert lib.odpd_abi_version() == _lib.ABI_VERSION == 13
    import opendpd_amd
    for name in ("fit_pa", "fit_dpd", "gmp_gram", "solve_ridge", "fit_gmp"):
        assert name in opendpd_amd.__all__ and callable(getattr(opendpd_amd, name)), name


def test_workspace_query_and_refusals():
    _lib, lib = _lib_and_desc()
    gmp = lambda hidden=11, bits_w=0, bits_a=0, flags=0: _lib.ModelDesc(_lib.BACKBONE_IDS["gmp"], hidden, 0, 0, bits_w, bits_a, flags)
    ws = lambda d, B, T: int(lib.odpd_gmp_gram_workspace_bytes(C.byref(d), B, T))
    shapes = [(1, 1), (1, 2), (3, 37), (64, 50), (1, 23040), (1, 1000000), (7, 1000000)]
    sizes = [ws(gmp(), B, T) for B, T in shapes]
    assert all(s > 0 and s % (496 * 496 * 8) == 0 for s in sizes), sizes
    assert sizes == sorted(sizes), sizes                                   # monotone in B * T
    assert sizes[-1] < 2 ** 30                                             # bounded: the samples' sums stay in registers
    bad = [_lib.ModelDesc(_lib.BACKBONE_IDS["dgru"], 11, 0, 0, 0, 0, 0), gmp(hidden=12), gmp(bits_w=8), gmp(bits_w=8, bits_a=8),
           gmp(flags=_lib.FLAG_INIT_STATE)]
    one = C.c_void_p(8)      # (never dereferenced: every call below is refused before a launch)
    for d in bad:
        assert ws(d, 64, 50) == EUNSUPPORTED
        assert lib.odpd_gmp_gram(None, C.byref(d), one, one, 64, 50, one, one) == EUNSUPPORTED
    d = gmp()
    assert ws(d, 0, 50) == EINVAL and ws(d, 4, 0) == EINVAL and ws(d, -1, 5) == EINVAL
    assert lib.odpd_gmp_gram(None, C.byref(d), one, one, 64, 50, None, one) == EINVAL      # null gram
    assert lib.odpd_gmp_gram(None, C.byref(d), one, one, 0, 50, one, one) == EINVAL        # B = 0
    assert lib.odpd_gmp_gram(None, C.byref(d), None, one, 64, 50, one, one) == EINVAL
    assert lib.odpd_gmp_gram(None, C.byref(d), one, None, 64, 50, one, one) == EINVAL
    assert lib.odpd_gmp_gram(None, C.byref(d), one, one, 64, 50, one, None) == EINVAL
    assert lib.odpd_gmp_gram(None, None, one, one, 64, 50, one, one) == EINVAL
