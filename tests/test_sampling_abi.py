"""The sampler entry points refuse out-of-range sizes with SPNERF_E_ARG before any launch (no GPU
needed: the pointers are never read)."""
import ctypes

import pytest

from spnerf_amd import _lib

E_ARG = -1
BUF = ctypes.create_string_buffer(64)
P = ctypes.c_void_p(ctypes.addressof(BUF))       # non-null: the size check is what refuses


@pytest.mark.parametrize("n", [1, 129, 0, -1])
def test_sample_guided_sizes(n):
    L = _lib.lib()
    assert L.spnerf_sample_guided(4, n, P, P, P, P, None, None, 2, None, P, None, P, P, None, None) == E_ARG
    assert b"n_samples" in L.spnerf_last_error()


@pytest.mark.parametrize("n", [1, 257, 0])
def test_sample_3sigma_sizes(n):
    L = _lib.lib()
    assert L.spnerf_sample_3sigma(4, n, P, P, P, P, P, None) == E_ARG
    assert b"sample_3sigma: n " in L.spnerf_last_error()


@pytest.mark.parametrize("nb,n_imp", [(0, 8), (256, 8), (8, 0)])
def test_sample_pdf_sizes(nb, n_imp):
    L = _lib.lib()
    assert L.spnerf_sample_pdf(4, nb, P, P, n_imp, P, 1e-5, P, None, None) == E_ARG
    assert b"out of range" in L.spnerf_last_error()


@pytest.mark.parametrize("S,stride", [(1, 8), (64, 7)])
def test_sample_stratified_sizes(S, stride):
    L = _lib.lib()
    assert L.spnerf_sample_stratified(4, S, P, stride, P, P, None, None) == E_ARG
    assert b"bad sizes" in L.spnerf_last_error()
