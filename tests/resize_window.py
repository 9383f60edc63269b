"""A second statement of the area filter of qoimi_decode_resized (qoi_amd/resize.py: resize is the normative one), for rectangles far too large
for that model's dense ``ow x cw`` weight matrices, and the images and items of tests/test_gpu_resize_wide.py.  Test helper only: numpy, no GPU,
no library.

The statement goes by WINDOWS.  Output pixel (X, Y) of an item ``cw x rh -> ow x oh`` overlaps the rows ``[Y*rh // oh, ceil((Y+1)*rh / oh))`` and
the columns ``[X*cw // ow, ceil((X+1)*cw / ow))`` of its rectangle and nothing else; the weights inside the window come from the closed form
``min((X+1)*cw, (k+1)*ow) - max(X*cw, k*ow)``.  All output pixels are evaluated together, tap offset by tap offset (row offset dr, all column
offsets at once): one gather of the window's pixels and one int64 multiply-add per row offset - no ``ow x cw`` matrix, no einsum.  The sums are
kept per window COLUMN, so that besides ``N_c``, ``M_c`` and ``A`` of every output pixel the partial sums of the kernel's lanes (resize.split:
lane l holds the columns ``[k0 + l*c, + c)``) and of every aligned group of ``2**s`` lanes - what a lane holds after s butterfly steps - can be
read off: the device tests prove with them that they reach the magnitudes they claim.
"""
import numpy as np

from qoi_amd import resize
from qoi_amd.resize import ALPHA_WEIGHTED, FLIP_X, FLIP_Y, PLAIN

B32 = 1 << 32


def axis(n_src, n_out):
    """(index int64[n_out, n], weight int64[n_out, n]): the window of every output column (row) padded to the widest one, n <= 65; padding
    has weight 0 and names the last source column."""
    X = np.arange(n_out, dtype=np.int64)
    lo, hi = X * n_src // n_out, -(-(X + 1) * n_src // n_out)
    n = int((hi - lo).max())
    idx = lo[:, None] + np.arange(n, dtype=np.int64)[None, :]
    w = np.minimum((X + 1)[:, None] * n_src, (idx + 1) * n_out) - np.maximum(X[:, None] * n_src, idx * n_out)
    w = np.where(idx < hi[:, None], w, 0)
    assert w.min() >= 0 and np.all(w.sum(axis=1) == n_src) and np.all(w[:, 0] > 0) and n <= resize.taps(n_src, n_out)
    return np.minimum(idx, n_src - 1), w


class Window:
    """The sums of one item over ``D uint8[h, w, och]``: ``colN int64[oh, ow, n, och]`` and (4 channels) ``colM int64[oh, ow, n, 3]`` per window
    column, ``N``, ``M``, ``A`` per output pixel of the unflipped result, ``T``."""

    def __init__(self, D, rect, out_size):
        D = np.asarray(D)
        x, y, cw, rh = (int(v) for v in rect)
        ow, oh = (int(v) for v in out_size)
        if D.ndim != 3 or D.shape[2] not in (3, 4) or D.dtype != np.uint8:
            raise ValueError("Window: D must be uint8[h, w, 3 or 4]")
        if min(cw, rh, ow, oh) < 1 or x < 0 or y < 0 or x + cw > D.shape[1] or y + rh > D.shape[0] or cw > 64 * ow or rh > 64 * oh:
            raise ValueError("Window: not an item the call accepts")
        och = D.shape[2]
        R = D[y:y + rh, x:x + cw]
        cidx, cwgt = axis(cw, ow)
        ridx, rwgt = axis(rh, oh)
        self.cw, self.rh, self.ow, self.oh, self.och, self.T = cw, rh, ow, oh, och, cw * rh
        self.colN = np.zeros((oh, ow, cidx.shape[1], och), dtype=np.int64)
        self.colM = np.zeros((oh, ow, cidx.shape[1], 3), dtype=np.int64) if och == 4 else None
        for dr in range(ridx.shape[1]):
            P = R[ridx[:, dr][:, None, None], cidx[None, :, :]].astype(np.int64)           # [oh, ow, n, och]: row offset dr of every window
            wgt = (rwgt[:, dr][:, None, None] * cwgt[None, :, :])[..., None]
            self.colN += wgt * P
            if och == 4:
                self.colM += wgt * (P[..., :3] * P[..., 3:4])
        self.N = self.colN.sum(axis=2)
        self.M = self.colM.sum(axis=2) if och == 4 else None
        self.A = self.N[..., 3] if och == 4 else None
        assert self.N.max() <= 255 * self.T and (och == 3 or self.M.max() <= 255 * 255 * self.T)

    # ------------------------------------------------------------------ the result
    def pixels(self, flags=0, mode=PLAIN, och=None):
        """uint8[oh, ow, och]: the rounded divisions as the docstring of qoi_amd/resize.py states them, then the flips.  och 3 of a window over
        4 channels: the colours alone (a decode at 3 channels drops the alpha), always PLAIN."""
        och = och or self.och
        if flags & ~(FLIP_X | FLIP_Y) or mode not in (PLAIN, ALPHA_WEIGHTED) or och not in (3, self.och):
            raise ValueError("pixels: flags, mode or och")
        T = self.T
        out = ((self.N + T // 2) // T)[..., :och]
        if mode == ALPHA_WEIGHTED and och == 4:
            A = self.A[..., None]
            out[..., :3] = np.where(A > 0, (self.M + A // 2) // np.maximum(A, 1), out[..., :3])
        assert out.min() >= 0 and out.max() <= 255
        out = out.astype(np.uint8)
        if flags & FLIP_Y:
            out = out[::-1]
        if flags & FLIP_X:
            out = out[:, ::-1]
        return np.ascontiguousarray(out)

    # ------------------------------------------------------------------ what the device holds on the way
    def lane_sums(self, col):
        """col[oh, ow, n, ch] -> int64[oh, ow, L, ch]: what lane l of an output pixel has added up before any exchange"""
        lg, c = resize.split(self.cw, self.ow)
        L = 1 << lg
        assert L * c >= col.shape[2]
        pad = np.zeros(col.shape[:2] + (L * c - col.shape[2], col.shape[3]), dtype=np.int64)
        return np.concatenate([col, pad], axis=2).reshape(col.shape[0], col.shape[1], L, c, col.shape[3]).sum(axis=3)

    def levels(self, col):
        """[level 0, ..., level lg]: level s is int64[oh, ow, L >> s, ch], the sums of the aligned groups of 2**s lanes - what the lanes hold
        after s butterfly steps; level lg is the pixel's sum."""
        out = [self.lane_sums(col)]
        while out[-1].shape[2] > 1:
            v = out[-1]
            out.append(v[:, :, 0::2] + v[:, :, 1::2])
        return out

    def divisions(self, mode):
        """every (n, d) the device divides for this item at 4 output channels (3: the PLAIN ones of the colours), as two flat int64 arrays:
        (N_c + T/2, T), and in the weighted mode (M_c + A/2, A) for the colours where A > 0"""
        T = self.T
        if mode == PLAIN or self.och == 3:
            n = (self.N + T // 2).reshape(-1)
            return n, np.full_like(n, T)
        A = self.A
        some = A > 0
        n = np.concatenate([(self.N[..., 3] + T // 2).reshape(-1), (self.N[..., :3][~some] + T // 2).reshape(-1), (self.M[some] + (A[some] // 2)[:, None]).reshape(-1)])
        d = np.concatenate([np.full(A.size + 3 * int((~some).sum()), T, dtype=np.int64), np.repeat(A[some], 3)])
        return n, d


def resized(D, rect, out_size, flags=0, mode=PLAIN):
    """what resize.resize returns, by windows"""
    return Window(D, rect, out_size).pixels(flags, mode)


def division_classes(n, d):
    """which of the paths of qoi_resize_core.h: resize_div_round / resize_div the pairs take"""
    n, d = np.asarray(n), np.asarray(d)
    pow2 = (d & (d - 1)) == 0
    return {"both below 2^32": bool(((n < B32) & (d < B32) & ~pow2).any()), "n from 2^32, d below": bool(((n >= B32) & (d < B32) & ~pow2).any()),
            "d from 2^32": bool(((d >= B32) & ~pow2).any()), "d a power of two, n from 2^32": bool((pow2 & (n >= B32)).any()),
            "d a power of two, n below 2^32": bool((pow2 & (n < B32)).any())}


# ---------------------------------------------------------------------------------- the images of tests/test_gpu_resize_wide.py
WIDE = (1040, 260)
HUGE = (4608, 3840)
HALF = (0, 0, 4096, 2048)                 # alpha exactly 128: T = 2**23, A = 2**30
CLEAR = (2215, 2503)                      # rows of alpha 0, the whole width
DARK = (2700, 3000)                       # rows of alpha 3 and colours 0..9


def wide_image():
    """1040 x 260 x 4 of 0xFFFFFFFF with about 1 % of the pixels random: the largest sums, and a misplaced tap still changes a result"""
    w, h = WIDE
    rng = np.random.default_rng(1040)
    D = np.full((h, w, 4), 255, dtype=np.uint8)
    hit = rng.random((h, w)) < 0.01
    D[hit] = rng.integers(0, 256, size=(int(hit.sum()), 4), dtype=np.uint8)
    return D


def huge_image():
    """4608 x 3840 x 4, flat pieces whose edges (multiples of 211, 173, 389 and 97) are no edges of output pixels: colours 246..255 (a mean
    above 243: N_c >= 2**32 over the whole image), alpha 255; alpha 128 in HALF; alpha 0 in the rows CLEAR; alpha 3 over colours 0..9 in the
    rows DARK; about 0.5 % random pixels outside HALF and CLEAR"""
    w, h = HUGE
    x, y = np.arange(w)[None, :], np.arange(h)[:, None]
    D = np.empty((h, w, 4), dtype=np.uint8)
    D[..., 0] = 246 + (x // 211 + y // 173) % 10
    D[..., 1] = 246 + (x // 211 + 2 * (y // 173) + 3) % 10
    D[..., 2] = 246 + (x // 389 + y // 97 + 7) % 10
    D[..., 3] = 255
    D[DARK[0]:DARK[1], :, :3] -= 246
    D[DARK[0]:DARK[1], :, 3] = 3
    rng = np.random.default_rng(4608)
    hit = rng.random((h, w)) < 0.005
    hit[HALF[1]:HALF[3], HALF[0]:HALF[2]] = False
    hit[CLEAR[0]:CLEAR[1]] = False
    D[hit] = rng.integers(0, 256, size=(int(hit.sum()), 4), dtype=np.uint8)
    D[HALF[1]:HALF[3], HALF[0]:HALF[2], 3] = 128
    D[CLEAR[0]:CLEAR[1], :, 3] = 0
    return D


def wide_rects():
    """(x, y, cw, rh, ow, oh) of the items over `wide` (test 1 of the device module)"""
    return [(0, 0, 1040, 260, 100, 260),          # 12 taps, 4 lanes of 3 columns: one lane's weight is 3 * 100 * 260
            (0, 0, 520, 260, 9, 5),               # 16 lanes, each below 2**32, the pixel above
            (5, 0, 300, 260, 301, 263),           # an upscale: one lane, no exchange
            (17, 11, 777, 201, 31, 7)]            # odd origin, odd sizes: 8 lanes


def huge_rects():
    """(x, y, cw, rh, ow, oh) of the items over `huge` (test 2 of the device module)"""
    w, h = HUGE
    return [(0, 0, w, h, 72, 60),                                  # ratio exactly 64: 16 lanes of 4 columns
            (0, 0, w, h, 73, 61),                                  # 65 taps in both axes: 16 lanes of 5 columns
            HALF + (64, 32), HALF + (65, 33),                      # a shift for T and for A; the same T and A at 65 taps
            (100, DARK[0] + 10, 4400, 280, 70, 5),                 # inside the dark rows
            (33, CLEAR[0] + 5, 4500, 270, 75, 9)]                  # inside the rows of alpha 0


def high_half_classes(win):
    """(a lane's sum from 2**32 before any exchange; a pixel whose lanes are all below 2**32 with a sum from it; a pixel whose largest group
    sum crosses 2**32 at a butterfly step s with 0 < s < lg) of the weighted colour sums of an item"""
    lv = win.levels(win.colM)
    lg = len(lv) - 1
    top = [v.max(axis=(2, 3)) for v in lv]                                # per pixel and level: the largest group sum of any colour
    lane = bool((top[0] >= B32).any())
    late = bool(((top[0] < B32) & (top[lg] >= B32)).any())
    inner = any(bool(((top[s - 1] < B32) & (top[s] >= B32)).any()) for s in range(1, lg))
    return lane, late, inner


def box_thumbnail(D, f, mode=PLAIN):
    """thumbs.thumbnail for an image whose sides f divides, over 32-bit block sums (64 * 64 * 255 * 255 < 2**32) of reshaped views: a
    17.7 Mpx image takes a fraction of a second"""
    h, w, och = D.shape
    if h % f or w % f or not 1 <= f <= 64:
        raise ValueError("box_thumbnail: f must divide both sides")

    def sums(a):                                                        # slice by slice: rows of a block, then its columns
        rows = np.zeros((h // f, w, a.shape[2]), dtype=np.uint32)
        v = a.reshape(h // f, f, w, a.shape[2])
        for k in range(f):
            rows += v[:, k]
        v = rows.reshape(h // f, w // f, f, a.shape[2])
        out = np.zeros((h // f, w // f, a.shape[2]), dtype=np.uint32)
        for k in range(f):
            out += v[:, :, k]
        return out.astype(np.int64)

    cnt = f * f
    S = sums(D)
    out = (S + cnt // 2) // cnt
    if mode == ALPHA_WEIGHTED and och == 4:
        A = S[..., 3:4]
        W = sums(D[..., :3].astype(np.uint16) * D[..., 3:4])
        out[..., :3] = np.where(A > 0, (W + A // 2) // np.maximum(A, 1), out[..., :3])
    return out.astype(np.uint8)
