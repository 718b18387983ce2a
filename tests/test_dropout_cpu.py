"""Dropout in the WideResNet encoder without a GPU: the mask generator restated in numpy against the Philox-4x32-10 known
answers, the three C-ABI entry points (declared, exported, refusing bad arguments before any launch), and the constructor's
checks of drop_rate."""
import ctypes
import os
import re

import numpy as np
import pytest

from shot_vae_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sv_dropout_fwd", "sv_bn_bwd_apply_dropout", "sv_dropout_mask")

# ---- the mask definition of include/shotvae_hip.h (sv_dropout_args), restated -------------------------------------------
M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on uint32 arrays (broadcast); returns the four output words"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint32) for v in (c0, c1, c2, c3))
    k0, k1 = np.asarray(k0, dtype=np.uint32), np.asarray(k1, dtype=np.uint32)
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0, k1 = k0 + W0, k1 + W1
            p0 = M0 * c0.astype(np.uint64)
            p1 = M1 * c2.astype(np.uint64)
            h0, l0 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32)
            h1, l1 = (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
            c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
    return c0, c1, c2, c3


def thr_of(p):
    return int(float(p) * 4294967296.0)


def keep_mask(key, unit, thr, n):
    """keep bits of the elements 0 .. n-1 (flat NHWC index inside one group's tensor) for one int64 key"""
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    e = np.arange(n, dtype=np.uint64)
    q = e >> np.uint64(2)
    w = philox4x32_10(q.astype(np.uint32), (q >> np.uint64(32)).astype(np.uint32), np.uint32(unit), np.uint32(0),
                      np.uint32(k & 0xFFFFFFFF), np.uint32(k >> 32))
    r = np.choose((e & np.uint64(3)).astype(np.int64), w)
    return r >= np.uint32(thr)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32_10"""
    cases = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
             ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
             ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
              (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in cases:
        got = tuple(int(v) for v in philox4x32_10(*ctr, *key))
        assert got == want, ["%08x" % v for v in got]


def test_mask_restatement_keeps_about_one_minus_p():
    """(the numpy restatement the GPU tests compare the kernels with: 1 - p of the elements kept, within 5 sigma)"""
    n = 1 << 18
    for p in (0.1, 0.3, 0.5):
        k = keep_mask(0x0123456789ABCDEF, 3, thr_of(p), n)
        sigma = (p * (1 - p) / n) ** 0.5
        assert abs(k.mean() - (1 - p)) < 5 * sigma, (p, k.mean())


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "shotvae_hip.h")).read()
    declared = set(re.findall(r"\bint\s+(sv_\w+)\s*\(", src))
    assert set(ENTRY_POINTS) <= declared
    assert "sv_dropout_args" in src and "#define SV_ABI_VERSION 8" in src
    if not os.path.exists(L.LIB_PATH):
        L.build()
    lib = ctypes.CDLL(L.LIB_PATH)
    for n in ENTRY_POINTS:
        assert hasattr(lib, n), n
        assert n in L.EXPORTS
    assert ctypes.sizeof(L.SvDropoutArgs) == 24


def test_dropout_args_follow_the_definition():
    a = L.dropout_args(4096, 5, 0.3)
    assert a.thr == thr_of(0.3) == 1288490188 and a.unit == 5
    assert a.scale == np.float32(1.0 / 0.7)


def _err():
    return L.lib().sv_last_error().decode()


def test_argument_refusals_without_a_gpu():
    """every refusal happens on the host, before anything is launched (the pointers are never dereferenced)"""
    lib = L.lib()
    C = ctypes
    P = 4096
    ok = L.dropout_args(P, 0, 0.3)

    def fwd(a, C_=32, ld=32, dtype=L.SV_BF16, stats=P, replicas=1):
        return lib.sv_dropout_fwd(dtype, P, 1024, C_, ld, C.byref(a) if a is not None else None, P, stats, replicas, 1, None)

    assert fwd(None) != 0 and "missing" in _err()
    nok = L.dropout_args(None, 0, 0.3)
    assert fwd(nok) == -1 and "keys" in _err()
    assert fwd(ok, C_=36, ld=40) == -2 and "multiples of 8" in _err()
    for p in (0.0, 1.0, -0.1, 1.5):
        a = L.dropout_args(P, 0, 0.3)
        a.p = p
        assert fwd(a) == -1 and "outside (0, 1)" in _err(), p
    a = L.dropout_args(P, 0, 0.3)
    a.thr = thr_of(0.5)
    assert fwd(a) == -1 and "thr" in _err()
    a = L.dropout_args(P, 0, 0.3)
    a.scale = 2.0
    assert fwd(a) == -1 and "scale" in _err()
    assert fwd(ok, replicas=3) == -1 and "power of two" in _err()
    assert fwd(ok, dtype=7) == -1
    # the backward: the same checks, and no residual
    br = (L.SvBnBranch * 1)()
    br[0].g = br[0].bsums = br[0].gamma = P
    br[0].replicas = 1

    def bwd(a, residual=None, C_=32):
        return lib.sv_bn_bwd_apply_dropout(L.SV_BF16, 1024, C_, C_, P, P, P, 64.0, br, 1, residual, P, 1,
                                           C.byref(a) if a is not None else None, None)

    assert bwd(nok) == -1 and "keys" in _err()
    assert bwd(ok, residual=P) == -1 and "residual" in _err()
    assert bwd(ok, C_=36) == -2
    a = L.dropout_args(P, 0, 0.3)
    a.p = 1.0
    assert bwd(a) == -1 and "outside (0, 1)" in _err()
    # the mask
    assert lib.sv_dropout_mask(None, 0, thr_of(0.3), 1024, 32, 1, P, None) == -1 and "keys" in _err()
    assert lib.sv_dropout_mask(P, 0, thr_of(0.3), 1024, 12, 1, P, None) == -2
    assert lib.sv_dropout_mask(P, 0, thr_of(0.3), 1024, 32, 5, P, None) == -1 and "groups" in _err()


def _construct(p):
    import shot_vae_amd as S
    return S.VariationalAutoEncoder("wideresnet-10-1", num_input_channels=3, drop_rate=p, img_size=(32, 32),
                                    data_parallel=False, continuous_latent_dim=128, disc_latent_dim=10, small_input=True,
                                    compute_dtype="fp32")


@pytest.mark.parametrize("p", [-0.1, 1.5, float("nan")])
def test_constructor_rejects_out_of_range_drop_rate(p):
    with pytest.raises(ValueError):
        _construct(p)


def test_constructor_refuses_drop_rate_one():
    with pytest.raises(NotImplementedError, match="drop_rate == 1"):
        _construct(1.0)


def test_constructor_accepts_dropout_and_keeps_state_dict_keys():
    m0, m3 = _construct(0), _construct(0.3)
    assert m3.drop_rate == 0.3 and m3._engine.drop_rate == 0.3 and m3._plan.drop_rate == 0.3
    assert list(m0.state_dict().keys()) == list(m3.state_dict().keys())
    from shot_vae_amd.engine import Plan
    assert Plan("wideresnet-28-2", K=10).drop_rate == 0.0
