"""The MX fp8 few-shot search without a device: the two C entries are exported and bound, they refuse bad
arguments before any launch, and the numpy statement of tests/fewshot_fp8_ref.py holds the facts of
csrc/mxfp8.h's rule that need no GPU."""
import ctypes

import numpy as np
import pytest

from aaclip import _lib

import fewshot_fp8_ref as F8


def _buf(n):
    """A 64-byte aligned host buffer's address: the entries below must return before touching it."""
    raw = ctypes.create_string_buffer(n + 64)
    addr = (ctypes.addressof(raw) + 63) // 64 * 64
    return raw, ctypes.c_void_p(addr)


def test_symbols_exported_and_bound():
    lib = _lib.lib()
    for name in ("aaclip_unit_rows_fp8mx", "aaclip_bank_nn_fp8mx"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name]
    assert len(_lib.SIGNATURES["aaclip_unit_rows_fp8mx"]) == 11
    assert len(_lib.SIGNATURES["aaclip_bank_nn_fp8mx"]) == 16
    assert _lib.ABI_VERSION == 9 and lib.aaclip_abi_version() == 9  # additions only


def test_bad_arguments_return_1_without_a_device():
    lib = _lib.lib()
    keep, p = _buf(1 << 16)
    K = 768

    def rows(in_dtype=_lib.F32, x=p, ldx=K, q=p, ldq=K, sc=p, ld_sc=4, rnorm=p, n=3, cols=K):
        return lib.aaclip_unit_rows_fp8mx(in_dtype, x, ldx, q, ldq, sc, ld_sc, rnorm, n, cols, None)
    assert rows(cols=K + 64, ldx=K + 64, ldq=K + 64) == 1   # cols % 128 != 0
    assert rows(ld_sc=5) == 1                                # odd ld_sc
    assert rows(ld_sc=2) == 1                                # ld_sc < rows
    assert rows(x=None) == 1 and rows(q=None) == 1 and rows(sc=None) == 1 and rows(rnorm=None) == 1
    assert rows(in_dtype=_lib.FP8) == 1 and rows(n=-1) == 1 and rows(cols=0) == 1
    assert rows(ldx=K - 128) == 1 and rows(ldq=K - 128) == 1
    assert rows(in_dtype=_lib.F16, ldx=K + 4) == 1           # a row stride that is not 16-byte aligned
    assert rows(n=0) == 0                                    # no rows: nothing to do, as aaclip_l2_normalize

    def nn(M=3, Nb=5, k=K, Q=p, ldq=K, q_sc=p, ld_qsc=4, q_rn=p, R=p, ldr=K, r_sc=p, ld_rsc=6, r_rn=p, part=p,
           part_bytes=1 << 12):
        return lib.aaclip_bank_nn_fp8mx(M, Nb, k, Q, ldq, q_sc, ld_qsc, q_rn, R, ldr, r_sc, ld_rsc, r_rn, part,
                                        part_bytes, None)
    assert nn(k=K + 64, ldq=K + 64, ldr=K + 64) == 1         # K % 128 != 0
    assert nn(k=0) == 1
    assert nn(ld_qsc=5) == 1 and nn(ld_rsc=7) == 1           # odd ld_sc
    assert nn(ld_qsc=2) == 1 and nn(ld_rsc=4) == 1           # shorter than the rows
    assert nn(M=0) == 1 and nn(Nb=0) == 1 and nn(M=-4) == 1
    for name in ("Q", "q_sc", "q_rn", "R", "r_sc", "r_rn", "part"):
        assert nn(**{name: None}) == 1, name
    assert nn(ldq=K - 128) == 1 and nn(ldr=K + 8) == 1       # a short stride, a stride off 16 bytes
    assert nn(part_bytes=8) == 1                             # part [3][1] needs 12 bytes
    assert nn(Q=ctypes.c_void_p(p.value + 4)) == 1           # a misaligned operand
    del keep


def test_quantiser_reproduces_the_pinned_exponents():
    """The probes of tests/test_fp8_gpu.py::test_mx_exponent_rule_edges and the exponents it pins."""
    top = np.float32(448.0 * 2 ** 5)
    v = np.array([0.0, 448.0, 449.0, 447.9, 256.0, 1.0, top, np.nextafter(top, np.float32(np.inf)), 2.0 ** -120,
                  448.0 * 2.0 ** -126, 3e38, 2.0 ** 127], dtype=np.float32)
    x = np.zeros((12, 128), np.float32)
    x[:, 0], x[:, 1], x[:, 2] = v, np.float32(-0.37) * v, v / np.float32(3)
    codes, e = F8.mx_quantise(x)
    assert e[:, 0].tolist() == [0, 0, 1, 0, 0, -8, 5, 6, -126, -126, 120, 119]
    assert (e[:, 1] == 0).all()                              # the all-zero block
    assert codes[1, 0] == 126 and codes[2, 0] == 118         # 448 -> the largest code; 449 / 2 -> 224
    assert not (codes[0] & 0x7F).any()                      # zeros, of either sign
    sc = F8.scale_buffer(e, ld=14)
    assert sc.shape == (1, 14, 2) and np.array_equal(F8.exponents_of(sc, 12), e)


def test_designed_rows_round_trip():
    """Entries 0 or +-2^-k with a power-of-four sum of squares: e4m3-exact after the block scaling, so
    quantise -> dequantise is the identity on the unit row, and the stored norm is exactly 1."""
    rng = np.random.default_rng(0)
    K = 768
    x = np.zeros((40, K))
    for i in range(39):
        n = [1, 4, 16][i % 3]
        cols = rng.choice(K, n, replace=False)
        x[i, cols] = rng.choice([-1.0, 1.0], n) * 2.0 ** -[0, 1, 2][i % 3] * 2.0 ** (i % 5 - 2)  # any power-of-two norm
    codes, e, rnorm = F8.unit_rows(x)
    unit = x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)
    deq = F8.dequantise(codes, F8.scale_buffer(e))
    assert np.array_equal(deq, unit)
    assert (rnorm[:39] == 1.0).all() and rnorm[39] == 0.0 and not codes[39].any() and not e[39].any()
    assert set(np.unique(e[:39])) <= {0, -8, -9, -10}        # 1 -> 2^-8 * 256, 2^-1 -> 2^-9 * 256, 2^-2 -> 2^-10 * 256
    cos = F8.cosines(deq[:39], deq[:39])
    assert np.array_equal(np.diag(cos), np.ones(39)) and np.abs(cos).max() == 1.0
    assert np.array_equal(F8.bank_nn(deq, deq)[:39], np.ones(39)) and F8.bank_nn(deq, deq)[39] == 0.0
