"""The work table of the per-pixel GEMM kernel (pixgemm.hip; sv_debug_pixgemm_table) against a direct enumeration of
{(iy, ky): oy = 2 iy - 1 + ky}: ConvTranspose2d(4, 2, 1) forward at H = 1, 2, 4 and its data gradient at H = 2, 4, 8.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from shot_vae_amd import _lib as L
from shot_vae_amd import geometry as G

CIN, N = 64, 32


def table(g):
    npix = C.c_int(0)
    pixels, taps = (C.c_int * (64 * 4))(), (C.c_int * (64 * 16 * 4))()
    L.call("sv_debug_pixgemm_table", C.byref(g), C.byref(npix), pixels, taps)
    px = np.array(pixels[:]).reshape(64, 4)[:npix.value]
    tp = np.array(taps[:]).reshape(64, 16, 4)[:npix.value]
    return px, tp


def enumerate_pairs(h_small, transposed):
    """{output pixel: {(ky * 4 + kx, iy, ix)}} of ConvTranspose2d(4, 2, 1) h x h -> 2h x 2h (transposed) or of the 4x4 stride-2
    pad-1 convolution 2h x 2h -> h x h (its data gradient: the same pairs with the roles of the two maps swapped)"""
    big = 2 * h_small
    axis = [(s, k, b) for s in range(h_small) for k in range(4) for b in [2 * s - 1 + k] if 0 <= b < big]     # (small, k, big)
    out = {}
    for sy, ky, by in axis:
        for sx, kx, bx in axis:
            key, val = ((by, bx), (ky * 4 + kx, sy, sx)) if transposed else ((sy, sx), (ky * 4 + kx, by, bx))
            out.setdefault(key, set()).add(val)
    return out


def python_pack(g, master):
    """the packed weights as include/shotvae_hip.h defines them: per phase [N][ntap][Cin] at w_off, tap t = master tap torig[t]"""
    pack = np.zeros(G.packed_size(g), dtype=master.dtype)
    for ph in range(g.nphase):
        P = g.phase[ph]
        idx = [P.torig[t] for t in range(P.ntap)]
        blk = master[:, idx, :]
        pack[P.w_off:P.w_off + blk.size] = blk.reshape(-1)
    return pack


@pytest.mark.parametrize("transposed,h,pairs", [(True, 1, 4), (True, 2, 36), (True, 4, 196), (False, 1, 4), (False, 2, 36), (False, 4, 196)])
def test_table_lists_exactly_the_valid_taps(transposed, h, pairs):
    """h = side of the SMALLER map: the forward reads it (H = h), the data gradient writes it (H = 2 h)"""
    g = G.convT_like(5, h, h, CIN, N, 4, 2, 1) if transposed else G.conv_like(5, 2 * h, 2 * h, CIN, N, 4, 2, 1)
    px, tp = table(g)
    want = enumerate_pairs(h, transposed)
    hout = 2 * h if transposed else h
    assert len(px) == hout * hout == len(want)
    assert sorted((int(r[0]), int(r[1])) for r in px) == sorted(want)                   # every output pixel exactly once
    assert int(px[:, 3].sum()) == pairs == sum(len(v) for v in want.values())          # 4 / 36 of 64 / 196 of 256
    assert all(px[i, 3] >= px[i + 1, 3] for i in range(len(px) - 1)), "long K loops first"
    # distinct values per (n, master tap, c): an entry that points at the wrong slice of the pack reads another tap's values
    master = np.arange(N * 16 * CIN, dtype=np.int64).reshape(N, 16, CIN)
    pack = python_pack(g, master)
    for (oy, ox, ph, ntap), rows in zip(px, tp):
        P = g.phase[ph]
        assert (oy % g.osy, ox % g.osx) == (P.ooy, P.oox) or g.nphase == 1
        got = set()
        for t, iy, ix, off in rows[:ntap]:
            assert 0 <= t < P.ntap and off == P.w_off + t * CIN
            got.add((P.torig[t], int(iy), int(ix)))
            for n in (0, N - 1):
                sl = pack[off + n * P.ntap * CIN: off + n * P.ntap * CIN + CIN]
                assert (sl == master[n, P.torig[t]]).all()
        assert got == want[(int(oy), int(ox))] and len(got) == ntap
        assert (rows[ntap:] == -1).all()


@pytest.mark.parametrize("g", [G.convT_like(2, 8, 8, CIN, N, 4, 2, 1), G.conv_like(2, 16, 16, CIN, N, 4, 2, 1), G.conv_like(2, 8, 8, CIN, N, 3, 2, 1),
                               G.convT_like(2, 4, 4, CIN, N, 3, 1, 1), G.conv_like(2, 1, 1, CIN, N, 1, 1, 0)])
def test_other_geometries_are_declined(g):
    with pytest.raises(L.ShotVaeHipError):
        table(g)


def test_switch_bit_is_the_header_s():
    src = open(L.os.path.join(L.HERE, "..", "include", "shotvae_hip.h")).read()
    assert "SV_K_PIXGEMM = %d" % L.K_PIXGEMM in src
