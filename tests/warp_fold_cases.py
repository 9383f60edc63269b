"""The sweep of tests/test_gpu_warp_fold.py: items of qoimi_decode_warped that walk the fold of a tap index (qoi_amd/warp.py: fold;
qoi_warp_border_core.h: warp_fold_position) over its whole accepted range, built by ONE function for the GPU test, for the CPU test that keeps
it from passing vacuously, and - as (k, n, border) triples - for the host walk of tests/test_warp_border_core_host.py (no GPU here).

The images hold their own pixel index: pixel j of image i is ``(j & 255, j >> 8 & 255, j >> 16 | i << 6, 255)``, so a wrong byte names the
index that was read.  The warp sets no limit on a rectangle's width or height of its own - only the image's pixel count bounds it, and one row
of that many pixels is 1.6 GB -, so the long row and column have ``nearest.MAX_SIZE + 3`` = 16387 pixels (64 KiB): beyond the side every
tensor filter stops at, and the periods of the three borders - 32774, 32772, 16387 - are in the tens of thousands.

An item of the sweep has ``a = e = ONE``, ``b = d = 0`` and an output of 16 x 1 (the columns of a row are swept) or 1 x 16 (the rows of a
column); with ``c`` (or ``f``) ``= 2 * ONE * k0 + ONE // 2`` output pixel X of a ``NEAREST`` item reads the tap ``k0 + X``.  For the
samplings that blend the offset is ``2 * ONE * k0 + ONE``: the fraction is one half, so the bilinear taps ``k0 + X`` and ``k0 + X + 1`` both
have a weight (warp_fold_next across P), the bicubic taps begin at ``k0 + X - 1`` and all four have one, and the two sub-samples of ``SUPER2``
have the fractions 1/4 and 3/4.  With P the period of (n, border): ``k0 = q * P + r - 8``, so the 16 outputs cross a multiple of P (r = 0),
its neighbours and the mirror point (r = n - 1, n), and for q = -1 and q = 2 also ``k = -P`` and ``k = 2P``, where warp_fold_position
changes from its conditional add or subtract to the quotient estimate - lanes of one wavefront on either side."""
import numpy as np

from qoi_amd import nearest, warp
from qoi_amd.warp import BICUBIC, NEAREST, ONE, REFLECT, REFLECT_101, SUPER2, WRAP

ROW, COLUMN, SMALL, DOT = range(4)
WIDE = nearest.MAX_SIZE + 3
SHAPES = [(WIDE, 1, 4), (1, WIDE, 4), (7, 5, 4), (1, 1, 4)]
BORDERS = (REFLECT, REFLECT_101, WRAP)
SIZES = (1, 2, 3, 5, 7, WIDE)
OUT = 16
FILL = 0x40C08020
K_TOP = 1 << 40                         # every accepted tap index lies inside (-K_TOP, K_TOP)
assert all(w * h < 1 << 16 for w, h, _ in SHAPES) and WIDE > nearest.MAX_SIZE and WIDE % 2 == 1


def pixels():
    """uint8[h, w, 4] per image: a pixel is its own index and its image's number"""
    out = []
    for i, (w, h, _) in enumerate(SHAPES):
        j = np.arange(w * h, dtype=np.int64)
        out.append(np.stack([j & 255, (j >> 8) & 255, (j >> 16) | (i << 6), np.full_like(j, 255)], axis=-1).astype(np.uint8).reshape(h, w, 4))
    return out


def period(n, border):
    return {REFLECT: 2 * n, REFLECT_101: max(2 * n - 2, 1), WRAP: n}[border]


def offset_of(k0, sampling):
    return 2 * ONE * k0 + (ONE // 2 if sampling & NEAREST else ONE)


def accepted(it):
    i = it[0]
    return warp.size(SHAPES[i][0], SHAPES[i][1], it, 4) != 0


def quotients(P, thinned, r_max=None):
    """the q of k0 = q * P + r - 8.  Full: 0, +-1, +-2, +-3, +-1000, +-(2**39 // P) and the largest and smallest q for which every r gives an
    accepted offset (|c| < 2**56; every tap index then lies inside |k| < 2**40).  Thinned: +-2, +-1000, +-(2**39 // P)."""
    far = (1 << 39) // P
    if thinned:
        return sorted({2, -2, 1000, -1000, far, -far})
    k_max = (warp.MAX_OFFSET - 1 - ONE) >> 17                          # the largest k0 whose offset of either kind is accepted
    k_min = -((warp.MAX_OFFSET - 1) >> 17)
    top, bottom = (k_max + 8 - (P - 1 if r_max is None else r_max)) // P, -((-(k_min + 8)) // P)
    assert accepted(warp.item(DOT, (0, 0, 1, 1), (OUT, 1), (ONE, 0, offset_of(k_max, 0), 0, ONE, 0), 0, 0))
    assert not accepted(warp.item(DOT, (0, 0, 1, 1), (OUT, 1), (ONE, 0, offset_of(k_max + 1, 0), 0, ONE, 0), 0, 0))
    assert accepted(warp.item(DOT, (0, 0, 1, 1), (OUT, 1), (ONE, 0, offset_of(k_min, NEAREST), 0, ONE, 0), 0, 0))
    return sorted({0, 1, -1, 2, -2, 3, -3, 1000, -1000, far, -far, top, bottom})


def remainders(n, P):
    return sorted({0, 1, n - 1, n, P - 1})


def sweep(sampling=NEAREST, thinned=False):
    """[(item, (k0x, k0y), (n, border, axis))]: the items of one sampling - ``NEAREST`` (the full sweep unless thinned), 0 (bilinear), ``BICUBIC``
    or ``SUPER2`` - in the order of the call.  Output pixel (X, Y) has its first tap - the only one of ``NEAREST`` - at (k0x + X, k0y + Y),
    the bicubic one a column and a row before that.  What the API rejects (|c| or |f| from 2**56: only at +-(2**39 // P)) is dropped."""
    out = []
    for border in BORDERS:
        for n in SIZES:
            P = period(n, border)
            for axis, image in ((0, ROW), (1, COLUMN)):
                at = 0 if n == WIDE else 11
                for q in quotients(P, thinned, max(remainders(n, P))):
                    for r in remainders(n, P):
                        k0 = q * P + r - 8
                        if axis == 0:
                            it = warp.item(image, (at, 0, n, 1), (OUT, 1), (ONE, 0, offset_of(k0, sampling), 0, ONE, 0), border | sampling, FILL)
                        else:
                            it = warp.item(image, (0, at, 1, n), (1, OUT), (ONE, 0, 0, 0, ONE, offset_of(k0, sampling)), border | sampling, FILL)
                        if accepted(it):
                            out.append((it, (k0, 0) if axis == 0 else (0, k0), (n, border, axis)))
        # both axes at once: the 7 x 5 image with a far row under every swept column, and the image of one pixel
        for image, (cw, rh) in ((SMALL, (7, 5)), (DOT, (1, 1))):
            Px, Py = period(cw, border), period(rh, border)
            for q in quotients(Px, True):
                for r in remainders(cw, Px):
                    k0, kf = q * Px + r - 8, -(q * Py + 3)
                    it = warp.item(image, (0, 0, cw, rh), (OUT, 2), (ONE, 0, offset_of(k0, sampling), 0, ONE, offset_of(kf, sampling)), border | sampling, FILL)
                    if accepted(it):
                        out.append((it, (k0, kf), ((cw, rh), border, 2)))
    return out


def direct(D, it, first):
    """uint8[oh, ow, och] of a ``NEAREST`` item of the sweep by plain indexing: pixel (X, Y) is R[fold(k0y + Y), fold(k0x + X)]"""
    _, x, y, cw, rh, ow, oh, flags = it[:8]
    border = flags & warp.BORDERS
    kx = warp.fold(first[0] + np.arange(ow, dtype=np.int64), cw, border)
    ky = warp.fold(first[1] + np.arange(oh, dtype=np.int64), rh, border)
    return D[y:y + rh, x:x + cw][ky[:, None], kx[None, :]]


def fold_triples(cases, before=0, taps=1):
    """sorted (k, n, border) of every tap index an axis of the cases folds: k0 - before .. k0 + 15 + taps - 1 of the swept axis (the other
    axis folds k = 0 and, for the samplings that blend, its neighbours: in the list as well)"""
    out = set()
    for it, first, _ in cases:
        _, _, _, cw, rh, ow, oh, flags = it[:8]
        for k0, n, m in ((first[0], cw, ow), (first[1], rh, oh)):
            out.update((k, n, flags & warp.BORDERS) for k in range(k0 - before, k0 + m + taps - 1))
    return sorted(out)


def host_triples():
    """what the host walk folds: every tap of the full ``NEAREST`` sweep and of the thinned bilinear (two taps) and bicubic (four, the first
    one before) sweeps"""
    return sorted(set(fold_triples(sweep())) | set(fold_triples(sweep(0, True), 0, 2)) | set(fold_triples(sweep(BICUBIC, True), 1, 4)))


SAMPLINGS_THINNED = (0, BICUBIC, SUPER2)
