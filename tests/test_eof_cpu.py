"""EOF analysis without a GPU: the public names and signatures, the host finish of the fit (ordering, sign rule, A, variances)
against numpy's SVD, the limits, and the C ABI of csrc/eof.hip (struct layout, argument checks)."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from downgan_amd import _lib, eof
from downgan_amd.GAN import losses
from tests import eof_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_and_reference_parameter_lists():
    assert list(inspect.signature(losses.eof_loss).parameters) == ["X", "hr", "fake", "device"]
    assert list(inspect.signature(losses.low_pass_eof_batch).parameters) == ["Z", "pcas", "fine", "transformer", "device", "fake"]
    assert inspect.signature(losses.low_pass_eof_batch).parameters["fake"].default is False
    assert list(inspect.signature(eof.get_eofs_and_project).parameters)[:2] == ["ncomp", "X"]
    for name in ("EOF", "EOFChannel", "host_finish", "sign_rule", "check_limits"):
        assert hasattr(eof, name), name


def _svd_reference(X, K):
    """sklearn's PCA(svd_solver="full") in numpy: components (svd_flip, u_based_decision=False), variance, ratio."""
    Xc = X - X.mean(0)
    U, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    i = np.argmax(np.abs(Vt), axis=1)
    Vt = Vt * np.sign(Vt[np.arange(Vt.shape[0]), i])[:, None]
    var = S ** 2 / (X.shape[0] - 1)
    return Vt[:K], var[:K], (S ** 2 / np.sum(S ** 2))[:K], Xc


@pytest.mark.parametrize("T,H,W,K", [(77, 60, 76, 13), (100, 64, 64, 20), (5, 3, 7, 4)])
def test_host_finish_matches_numpy_svd(T, H, W, K):
    X = eof_fixture.fields(0, T, 1, H, W)[:, 0].reshape(T, H * W).numpy()
    Vt, var, ratio, Xc = _svd_reference(X, K)
    G = Xc @ Xc.T
    lam, A, v, r = eof.host_finish(G, K)
    assert np.all(np.diff(lam) < 0)                              # descending
    assert A.shape == (K, T)
    E = eof.sign_rule(A @ Xc)
    np.testing.assert_allclose(v, var, rtol=1e-9)
    np.testing.assert_allclose(r, ratio, rtol=1e-9)
    np.testing.assert_allclose(np.linalg.norm(E, axis=1), 1.0, atol=1e-9)
    np.testing.assert_array_equal(np.sign(E[np.abs(Vt) > 1e-6]), np.sign(Vt[np.abs(Vt) > 1e-6]))   # signs exactly
    np.testing.assert_allclose(E, Vt, atol=1e-7)


def test_sign_rule_ties_go_to_the_lowest_index():
    E = np.array([[0.5, -0.5, 0.1], [-0.2, 0.2, -0.7], [0.0, 0.0, 0.0]])
    out = eof.sign_rule(E)
    np.testing.assert_array_equal(out, [[0.5, -0.5, 0.1], [0.2, -0.2, 0.7], [0.0, 0.0, 0.0]])


@pytest.mark.parametrize("T,C,K,limit", [(1, 2, 1, "T <="), (8193, 2, 20, "T <="), (100, 9, 20, "C <="), (100, 2, 0, "n_components"),
                                         (100, 2, 100, "n_components"), (100, 2, 65, "n_components"), (10, 1, 10, "T - 1")])
def test_limits_raise_value_error(T, C, K, limit):
    with pytest.raises(ValueError, match=limit.replace("(", r"\(")):
        eof.check_limits(T, C, K)


def test_fit_checks_limits_before_touching_a_device():
    with pytest.raises(ValueError, match="T <="):
        eof.EOF(1).fit(torch.zeros(1, 2, 4, 4))
    with pytest.raises(ValueError, match="C <="):
        eof.EOF(2).fit(torch.zeros(4, 9, 4, 4))
    with pytest.raises(ValueError, match="n_components"):
        eof.EOF(65).fit(torch.zeros(100, 1, 4, 4))


def test_eof_fields_struct_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls = _lib.EofFields
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT}/include/downgan_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(dg_eof_fields));']
    lines += [f'  printf("{f} %zu\\n", offsetof(dg_eof_fields, {f}));' for f, _ in cls._fields_]
    lines += ['  printf("maxc %d\\nmaxk %d\\n", DG_EOF_MAX_C, DG_EOF_MAX_K);', '  return 0;', '}']
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert (int(got["maxc"]), int(got["maxk"])) == (_lib.EOF_MAX_C, _lib.EOF_MAX_K) == (eof.C_MAX, eof.K_MAX)


def test_abi_rejects_bad_arguments_without_launching():
    lib = _lib.lib()
    ok = dict(base=0x1000, dtype=_lib.DG_F32, T=10, C=2, P=100, ld_t=200, ld_c=100, ld_p=1)
    f = lambda **kw: C.byref(_lib.EofFields(**dict(ok, **kw)))
    p = C.c_void_p(0x2000)
    assert lib.dg_eof_mean(f(base=0), p, None) == -1
    assert lib.dg_eof_mean(f(C=9), p, None) == -1
    assert lib.dg_eof_mean(f(dtype=5), p, None) == -2
    assert lib.dg_eof_gram(f(), p, 0, p, p, None) == -1                 # nslice < 1
    assert lib.dg_eof_gram(f(), p, 3, p, p, None) == -1                 # nslice > ceil(P / 64)
    assert lib.dg_eof_gram(f(), None, 1, p, p, None) == -1
    assert lib.dg_eof_components(f(), p, p, 65, p, 100, 6500, p, None) == -1
    assert lib.dg_eof_components(f(), p, p, 0, p, 100, 6500, p, None) == -1
    assert lib.dg_eof_flip(None, 2, 4, 100, 100, 400, p, None) == -1
    assert lib.dg_eof_project(f(), None, p, 4, 100, 400, 0, p, p, None) == -1
    assert lib.dg_eof_project(f(dtype=_lib.DG_BF16), None, None, 4, 100, 400, 1, p, p, None) == -1
    assert lib.dg_eof_reconstruct(p, 0, 2, 4, p, 100, 400, 100, None, p, None) == -1
    assert lib.dg_eof_reconstruct(p, 2, 2, 4, p, 100, 400, 100, None, None, None) == -1
