"""``qoimi_decode_warped`` as pure functions - the normative statement of the result (what warp_gather of qoi_warp.hip computes from the decoded
pixels of an image), of the staging plan, of ``qoimi_warp_orient`` and of the kernel's tiles (plain numpy / integer arithmetic, no GPU).

An item is ``(image, x, y, width, height, out_width, out_height, flags, a, b, d, e, fill, reserved, c, f)`` - the fields of ``qoimi_warp`` in
their order; an ``api.QoimiWarp`` is taken as well.  With D the decode of stream ``image`` as ``uint8[h, w, och]`` (a 3-channel decode has
alpha 255), ``R = D[y:y+height, x:x+width]``, ``cw = width``, ``rh = height``, ``ow = out_width``, ``oh = out_height``; all arithmetic is
integer, every shift and division floors.

* Coordinates are DOUBLED pixel-centre coordinates with 16 fractional bits: the centre of source column k of R lies at ``(2k + 1) << 16``.
* Output pixel (X, Y) has ``U = 2X + 1``, ``V = 2Y + 1``.  The item carries the INVERSE map, from the output into R:
  ``Px = a*U + b*V + c``, ``Py = d*U + e*V + f``.  The identity is ``a = e = 65536`` (``ONE``) with everything else 0.
* Bilinear over 2 x 2 samples: ``px = Px - 65536``, ``k0 = px >> 17``, ``fx = px & 131071``; columns ``k0`` and ``k0 + 1`` have the weights
  ``131072 - fx`` and ``fx``; rows likewise from Py.  A sample with a weight of 0 counts as not taken.
* Samples outside R are never read, even where the image has pixels there: with ``REPLICATE`` their indices are clamped into R, otherwise
  they take ``fill`` (``r | g << 8 | b << 16 | a << 24``; a 3-channel output ignores its alpha).
* With ``NEAREST`` (a flag, combinable with ``REPLICATE``) the 2 x 2 taps are replaced by ONE sample - selection, for label maps: column
  ``k = Px >> 17``, row ``r = Py >> 17`` (they floor for negative values); column k covers ``[k << 17, (k + 1) << 17)``, its centre at
  ``(2k + 1) << 16``.  Where k is outside ``[0, cw)`` or r outside ``[0, rh)`` the index is clamped into R with ``REPLICATE``, else the output
  pixel is ``fill`` (a 3-channel output ignores its alpha).  The output pixel is the sample, byte for byte, in both modes.  With the
  identity that is ``crops.crop``; with any ``orient`` item it equals the bilinear result, every position being a pixel centre.
* With ``BICUBIC`` (a flag, combinable with ``REPLICATE``, never with ``NEAREST``) the 2 x 2 taps are replaced by 4 x 4 samples under Keys' cubic
  with a = -1/2 - the kernel of ``bicubic.py`` (PIL ``BICUBIC``), not the a = -3/4 of ``cv2.INTER_CUBIC`` and torch's ``grid_sample``.  The
  position is the bilinear warp's.  One axis, ``u = 2**17``: ``p = P - 65536``, ``k0 = p >> 17``, ``fr = p & 131071``; the samples are
  ``k0 - 1, k0, k0 + 1, k0 + 2`` at the distances ``d = u + fr, fr, u - fr, 2u - fr``; ``c(d) = 3d^3 - 5u*d^2 + 2u^3`` for ``d <= u``,
  ``-d^3 + 5u*d^2 - 8u^2*d + 4u^3`` for ``u < d < 2u``, 0 from ``2u`` on (every term below ``2**56``).  The four c add up to
  ``W = 2u^3 = 2**52`` for every fr (asserted here).  ``q_j = (c_j + 2**36) >> 37``; the deficit ``2**15 - sum q_j`` goes to the tap with
  the largest c, the lowest j on a tie: the weights of an axis add up to ``2**15``.  A tap with ``q == 0`` counts as not taken.  With
  ``REPLICATE`` each of the four indices is clamped into R, else a sample outside R has the value ``fill`` and KEEPS its weight (no
  renormalisation, as in the bilinear warp).  ``N_c = sum qy * qx * c`` over the 4 x 4 samples - two axes, one rounding.  ``PLAIN``: every
  channel is ``clamp((N_c + 2**29) >> 30, 0, 255)``.  ``ALPHA_WEIGHTED``, 4 channels only: ``A = N_a``, alpha is the PLAIN value; where
  ``A > 0`` r, g and b are ``clamp((sum qy*qx*c*a + A // 2) // A, 0, 255)``, where ``A <= 0`` (the negative lobes make that possible) they
  are the PLAIN value.  ``sum |q|`` of an axis is at most ``5 * 2**13`` (1.25 * 2**15, reached at fr = u / 2; asserted here), so a
  horizontal blend is below ``2**24``, ``|N_c| < 2**40`` and the alpha-weighted sums are below ``2**48``.
  At a pixel centre (fr = 0 on both axes) the weights are ``(0, 2**15, 0, 0)``: the identity is ``crops.crop`` and every ``orient`` item
  equals the bilinear result.  A constant stays the constant under any map with ``REPLICATE``.  With ``a = e = ONE // s``, s a power of two,
  everything else 0 and an output of s times the rectangle, every output pixel whose 4 x 4 taps lie inside R equals ``bicubic.bicubic``
  enlarging by s (the same rational weights; at the border the filter renormalises and the warp replicates).
  Against a float64 evaluation of the same kernel with the same border rule (``cubic_reference``), PLAIN: the derivation of ``bicubic.py``
  with T = 4 taps and L = sum |w| <= 3/2 per axis gives ``E = 255 / 2**16 * 9 + 255 * 9 / 2**31 < 0.036``: a byte differs from the rounded,
  clamped reference by at most ``floor(1 + E) = 1`` (``cubic_bound``), and only at a rounding boundary.
* With ``REFLECT`` = 64, ``REFLECT_101`` = 128 or ``WRAP`` = 256 (flags; with ``REPLICATE`` they are THE BORDER: at most one of the four, each
  combinable with ``NEAREST`` or with ``BICUBIC``) positions, ``k0``, fractions, weights (the bicubic deficit tap too), the one rounding, the
  clamp, the alpha-weighted mode and "a tap with weight 0 is not taken and never read" stay exactly as they are for all three samplings:
  only the INDEX of a tap changes.  Every 64-bit tap index k on an axis of n samples is folded into ``[0, n)`` before anything is narrowed
  (``fold``); ``fill`` is not used, as with ``REPLICATE``.  ``mod`` floors: ``0 <= m < P`` for negative k too.
  ``REFLECT`` ("dcba|abcd|dcba"; numpy ``symmetric``, ``cv2.BORDER_REFLECT``, torch ``reflection`` with ``align_corners=False``):
  ``P = 2n``, ``m = k mod P``, index ``m if m < n else P - 1 - m``.
  ``REFLECT_101`` ("dcb|abcd|cba"; numpy ``reflect``, ``cv2.BORDER_REFLECT_101``, torchvision ``Pad`` "reflect"): index 0 if ``n == 1``,
  else ``P = 2n - 2``, ``m = k mod P``, index ``m if m < n else P - m``.
  ``WRAP`` ("abcd|abcd|abcd"; numpy ``wrap``): index ``k mod n``.
  Each tap is folded on its own - the 2 of the bilinear sampling, the 4 of the bicubic, the one of ``NEAREST`` -, as ``cv2.warpAffine``
  does; for ``REFLECT`` that equals torch's reflection of the coordinate.  R is still what is staged and what the border is taken at:
  nothing outside R is ever read.  With the identity plus a whole-pixel translation into a larger output each border gives
  ``np.pad(R, mode=...)`` byte for byte in all three samplings, for pads larger than n and for ``n == 1`` too; a constant stays the
  constant; every pixel whose taps all lie inside R equals the call without the flag; the bounds against float64 are the unflagged ones.
* ``N_c = sum wy * wx * c`` over the four samples; the weights add up to ``2**34``.
* ``PLAIN``: every channel is ``(N_c + 2**33) >> 34`` - ONE rounding.
* ``ALPHA_WEIGHTED``, 4 channels only: ``A = N_a``; alpha as in the plain mode; where ``A > 0`` r, g and b are
  ``(sum wy*wx*c*a + A // 2) // A``, where ``A == 0`` they are the PLAIN value.  With 3 channels this mode is PLAIN.
* There is no antialiasing: a map that reduces still takes four samples (reduce first with ``resize.resize`` where that matters) - unless the
  item asks for supersampling:
* With ``SUPER2`` = 1024 (s = 2, L = 1) or ``SUPER4`` = 2048 (s = 4, L = 2) (flags; at most one of the two, with the bilinear sampling only -
  never with ``NEAREST`` or ``BICUBIC`` -, with the fill or any of the four borders; 512 is not a flag) output pixel (X, Y) is the mean of
  s x s bilinear samples laid on a regular grid inside the pixel, with ONE rounding.  For ``0 <= i, j < s``:
  ``Us = s*U + 2i + 1 - s``, ``Vs = s*V + 2j + 1 - s`` (the sub-sample's centre in coordinates s times finer),
  ``Px = ((a*Us + b*Vs) >> L) + c``, ``Py = ((d*Us + e*Vs) >> L) + f`` (the shift floors).  From (Px, Py) the 2 x 2 taps, their weights, their
  indices and the border are exactly those of the bilinear warp: a tap outside R takes ``fill``, under ``REPLICATE`` its index is clamped,
  under ``REFLECT`` / ``REFLECT_101`` / ``WRAP`` it is folded, each tap on its own; a tap of weight 0 is not taken and never read.
  ``N_c`` is the sum over all s**2 sub-samples and their four taps of ``wy * wx * c``.  ``PLAIN``: every channel is
  ``(N_c + 2**(33 + 2L)) >> (34 + 2L)``.  ``ALPHA_WEIGHTED`` with 4 channels: ``A = N_a``, alpha is the PLAIN value; where ``A > 0`` r, g and
  b are ``(M_c + A // 2) // A`` with ``M_c`` the same sum of ``wy * wx * c * a``; where ``A == 0`` they are the PLAIN value.  With 3 channels
  this mode is PLAIN.  Bounds: ``Us, Vs < 2**23``, so ``|a*Us + b*Vs| < 2**55``; ``|Px|, |Py| < 2**57`` as without the flag, so the fold's
  preconditions hold unchanged; ``N_c <= 255 * 2**38 < 2**46``; ``M_c < 2**54``.
  With ``a = e = s * ONE``, ``b = c = d = f = 0`` and an output of ``(cw / s) x (rh / s)``, s dividing both, every sub-sample is a pixel
  centre: the item is the exact s x s box average with one rounding and equals ``thumbs.thumbnail`` at factor s and ``resize.resize`` of the
  same rectangle byte for byte in both modes (the common factor ``2**34`` cancels in ``(S + cnt // 2) // cnt`` and ``(W + A // 2) // A``).
  A constant rectangle stays the constant under any map with any of the four borders.  The result differs by at most 1 from a float64
  evaluation of the same s**2 positions (``super_reference``: taken from the integer Px, Py, bilinear, same border rule, averaged, rounded
  once), and only where the float value lies at a rounding boundary, because ``N_c`` is exact.  There is NO adaptivity: the flag takes s**2
  sub-samples whether or not the map reduces, and beyond 4 : 1 the result still aliases.
* With ``VOTE2`` = 8192 (s = 2, L = 1) or ``VOTE4`` = 16384 (s = 4, L = 2) (flags; a fourth sampling: at most one of the two, never with
  ``NEAREST``, ``BICUBIC``, ``SUPER2`` or ``SUPER4``, with the fill or any one of the four borders; 4096 is not a flag) output pixel (X, Y) is
  the MAJORITY VOTE of s x s nearest sub-samples - for label maps under a map that reduces, where ``NEAREST`` looks at one source pixel per
  output pixel.  For ``0 <= i, j < s`` the positions ``Us``, ``Vs``, ``Px``, ``Py`` are exactly those of ``SUPER2`` / ``SUPER4``, with their
  bounds.  The value of a sub-sample is that of ``NEAREST`` at (Px, Py): column ``k = Px >> 17``, row ``r = Py >> 17``; inside R it is
  ``R[r][k]``, all four bytes of the 4-channel decode (a 3-channel stream has alpha 255); outside R each index is clamped under
  ``REPLICATE``, folded on its own under ``REFLECT`` / ``REFLECT_101`` / ``WRAP``, and without a border flag the value is the dword ``fill``
  as given, all four bytes.  A value votes as a whole dword; the count of a value is the number of the s**2 sub-samples equal to it; the
  winners are the values with the largest count.  One winner is the output; of several the centre value if it is a winner, otherwise the
  winner with the lowest key ``r << 24 | g << 16 | b << 8 | a`` - the vote and the tie rule of ``mode.mode``.  The centre value is what
  ``NEAREST`` gives this output pixel with the same border or fill, from ``Px = a*U + b*V + c``, ``Py = d*U + e*V + f``; it does not vote.
  Both modes give the same bytes; och 3 drops alpha after the vote.  Consequences: every output pixel is one of its sub-sample values;
  with the identity and every ``orient`` item all s**2 sub-samples fall into the pixel the centre falls into (at most 49152 < 65536 from a
  pixel centre), so the item is ``crops.crop``, respectively the ``NEAREST`` warp; with ``a = e = s * ONE``, ``b = c = d = f = 0`` and an
  output of ``(cw / s) x (rh / s)``, s dividing both, sub-sample (i, j) is source pixel (sX + i, sY + j) and the centre value pixel
  (sX + s/2, sY + s/2): the item is ``mode.mode`` for that rectangle and size and the MODE tile of ``tiles.py`` at factor s, byte for
  byte; a constant rectangle stays the constant under any map with any of the four borders; there is no adaptivity, and beyond 4 : 1 the
  result still skips pixels.  ``vote_reference`` is the same statement as a naive loop.

* With ``PROJECTIVE`` = 131072 (``1 << 17``; a flag; 32768 and 65536 are not flags) the map is a PERSPECTIVE map, a homography of the output
  rectangle.  The flag goes with the fill or any one of the four borders and with the bilinear sampling, ``NEAREST`` or ``BICUBIC``, never
  with ``SUPER2``, ``SUPER4``, ``VOTE2`` or ``VOTE4``.  With it ``reserved`` holds ``g = int16(reserved & 0xFFFF)`` and
  ``h = int16(reserved >> 16)``, two's complement (``proj_of``; ``item(..., proj=(g, h))`` packs them).  With ``ow, oh`` the output's size:
  ``L`` is the smallest integer >= 0 with ``2**L >= max(ow, oh)`` and ``F = 14 + L`` (14..34, ``proj_bits``); ``Uc = U - ow``,
  ``Vc = V - oh`` (the doubled offsets from the output's centre); ``Nx = a*U + b*V + c``, ``Ny = d*U + e*V + f`` (the positions without the
  flag); ``W = 2**F + g*Uc + h*Vc`` (the denominator, 1.0 at the centre); ``Px = floor(Nx * 2**F / W)``, ``Py = floor(Ny * 2**F / W)``
  (``positions``).  From Px and Py on nothing changes.  The scale is the item's because ``W > 0`` needs ``|gamma| * ow < 1``: the useful range
  of g is ``1 / ow``, and 16 bits at ``F = 14 + L`` cover it at every size.  Limits, behind all others, in this order: the flag with a
  ``SUPER`` or ``VOTE`` flag; ``|c|`` or ``|f|`` from ``2**53``; ``2**F - |g|*(ow - 1) - |h|*(oh - 1) < 2**(F - 3)`` (the exact minimum of the
  linear W over the pixel grid: the denominator stays at or above 1/8).  Then ``|Nx| < 2**54``, ``2**(F-3) <= W < 5 * 2**F < 2**37`` and
  ``|Px| <= 8 * |Nx| < 2**57``.  With ``g = h = 0``, ``Px = Nx``: the bytes of the item without the flag.  The map applied is the quantised
  homography, exactly; against a float64 evaluation of that same map a bilinear value differs by at most 1, at a rounding boundary only
  (the position is floored by less than 2**-17 of a pixel); a constant stays the constant under ``REPLICATE``.  ``homography`` and
  ``perspective`` quantise a 3 x 3 matrix or four corner points and report what that costs at the output's corners.

Limits, in the order the C side checks them: a zero size; a rectangle that leaves its image; ``ow, oh < 2**20``; ``ow * oh < 400 000 000``;
``|c|, |f| < 2**56``; no flag bit but ``REPLICATE``, ``NEAREST``, ``BICUBIC``, ``REFLECT``, ``REFLECT_101``, ``WRAP``, ``SUPER2``, ``SUPER4``,
``VOTE2`` and ``VOTE4`` (2, 8, 32, 512 and 4096 are not flags), then not ``NEAREST`` and ``BICUBIC`` together, then not more than one of the
four borders, then not both ``SUPER`` flags, then no ``SUPER`` flag with ``NEAREST`` or ``BICUBIC``, then not both ``VOTE`` flags, then no
``VOTE`` flag with ``NEAREST``, ``BICUBIC`` or a ``SUPER`` flag (``PROJECTIVE`` is a flag too); ``reserved == 0`` without ``PROJECTIVE``, with
it the three limits above.  Then ``|a*U|, |b*V| <= 2**31 * 2**21 = 2**52`` and
``|Px|, |Py| < 2**57``; ``N_c <= 255 * 2**34 < 2**42``; the alpha-weighted sums are below ``2**50``: everything fits int64.

With the identity the result is ``crops.crop``; with ``a = ONE // s`` and REPLICATE it is ``bilinear.bilinear`` enlarging by the power of two s;
a constant stays the constant under any map with REPLICATE.

The plan is ``crops.plan`` over the items' ``(image, x, y, width, height)``: the caller keeps the rectangle tight around what the map reaches.

The tiles of the kernel: 16 x 16 output pixels, row-major over ``ceil(ow / 16) x ceil(oh / 16)``; work item t of a tile is its pixel
``(t & 15, t >> 4)`` (``place``), so a wavefront of 64 covers 16 columns x 4 rows at any angle of the map.
"""
from typing import Optional, Tuple

import numpy as np

from . import bicubic, crops, resize

REPLICATE = 1
NEAREST = 4                     # one sample, not 2 x 2 taps (2 is not a flag)
BICUBIC = 16                    # 4 x 4 samples under Keys' cubic, a = -1/2 (8 is not a flag)
REFLECT = 64                    # "dcba|abcd|dcba" (32 is not a flag)
REFLECT_101 = 128               # "dcb|abcd|cba"
WRAP = 256                      # "abcd|abcd|abcd"
BORDERS = REPLICATE | REFLECT | REFLECT_101 | WRAP   # at most one of them
SUPER2 = 1024                   # 2 x 2 bilinear sub-samples per output pixel, one rounding (512 is not a flag)
SUPER4 = 2048                   # 4 x 4
SUPERS = SUPER2 | SUPER4        # at most one of them, with the bilinear sampling only
VOTE2 = 8192                    # the majority vote of 2 x 2 nearest sub-samples per output pixel: for label maps (4096 is not a flag)
VOTE4 = 16384                   # 4 x 4
VOTES = VOTE2 | VOTE4           # at most one of them, a sampling of its own: with no other sampling and no SUPER flag
PROJECTIVE = 1 << 17            # a perspective map: reserved holds g and h; never with a SUPER or VOTE flag (32768 and 65536 are not flags)
PROJ_BASE = 14                  # F = PROJ_BASE + L: the fractional bits of the denominator
PROJ_MAX_OFFSET = 1 << 53       # |c|, |f| of an item with PROJECTIVE stay below it
CUBIC_ONE = bicubic.ONE         # the weights of an axis add up to it
CUBIC_L1_MAX = 5 << 13          # sum |q| of an axis stays at or below it
PLAIN = resize.PLAIN
ALPHA_WEIGHTED = resize.ALPHA_WEIGHTED
ONE = 1 << 16                   # a factor of 1; a pixel is 2 * ONE in doubled coordinates
MAX_OUT = 1 << 20               # out_width, out_height stay below it
MAX_AREA = 400_000_000          # out_width * out_height stays below it
MAX_OFFSET = 1 << 56            # |c|, |f| stay below it
TILE = 16
IDENTITY = (ONE, 0, 0, 0, ONE, 0)   # (a, b, c, d, e, f)


def fields(it) -> Tuple[int, ...]:
    """The sixteen fields of an item given as such a tuple or as a ``qoimi_warp`` structure, in the structure's order."""
    names = ("image", "x", "y", "width", "height", "out_width", "out_height", "flags", "a", "b", "d", "e", "fill", "reserved", "c", "f")
    if hasattr(it, "image"):
        return tuple(int(getattr(it, n)) for n in names)
    if len(it) != len(names):
        raise ValueError("fields: an item has sixteen fields")
    return tuple(int(v) for v in it)


def item(image: int, rect, out_size, matrix=IDENTITY, flags: int = 0, fill: int = 0, proj=None) -> Tuple[int, ...]:
    """An item's tuple from rect (x, y, width, height), out_size (out_width, out_height) and matrix (a, b, c, d, e, f); proj = (g, h), each
    16-bit signed, makes it a ``PROJECTIVE`` item: the flag is set and ``reserved`` holds the two (``proj_reserved``)."""
    x, y, cw, rh = rect
    ow, oh = out_size
    a, b, c, d, e, f = matrix
    if proj is None:
        return (image, x, y, cw, rh, ow, oh, flags, a, b, d, e, fill, 0, c, f)
    return (image, x, y, cw, rh, ow, oh, flags | PROJECTIVE, a, b, d, e, fill, proj_reserved(*proj), c, f)


def proj_reserved(g: int, h: int) -> int:
    """``reserved`` of a ``PROJECTIVE`` item: g in its lower and h in its upper 16 bits, two's complement."""
    if not (-2 ** 15 <= g < 2 ** 15 and -2 ** 15 <= h < 2 ** 15):
        raise ValueError("proj_reserved: g and h are 16-bit signed")
    return (int(g) & 0xFFFF) | ((int(h) & 0xFFFF) << 16)


def proj_of(reserved: int) -> Tuple[int, int]:
    """(g, h) of a ``PROJECTIVE`` item's ``reserved``."""
    g, h = reserved & 0xFFFF, (reserved >> 16) & 0xFFFF
    return g - ((g & 0x8000) << 1), h - ((h & 0x8000) << 1)


def proj_bits(ow: int, oh: int) -> int:
    """F of an ow x oh output: 14 + L with L the smallest integer >= 0 with 2**L >= max(ow, oh)."""
    return PROJ_BASE + (max(ow, oh) - 1).bit_length()


def _scaled_quotient(N: np.ndarray, W: np.ndarray, F: int) -> np.ndarray:
    """int64: floor(N * 2**F / W) for |N| < 2**54 and 0 < W < 2**37 without leaving int64 (the product has up to 88 bits): long division -
    the head floor(N / W), then the F fractional bits in chunks of at most 17, so that the remainder r < W shifted up stays below 2**54."""
    P = N // W                                                           # (numpy's // floors)
    r = N - P * W
    left = F
    while left:
        s = min(left, 17)
        t = r << s
        q = t // W
        r = t - q * W
        P = P * (1 << s) + q
        left -= s
    return P


def positions(out_size, matrix=IDENTITY, flags: int = 0, reserved: int = 0):
    """(Px, Py), int64[out_height, out_width] each: the position of every output pixel in the source rectangle in doubled coordinates with 16
    fractional bits - ``a*U + b*V + c`` and ``d*U + e*V + f``, and with ``PROJECTIVE`` those divided by the item's denominator:
    ``floor(N * 2**F / W)``, exactly.  Integers only."""
    ow, oh = (int(v) for v in out_size)
    a, b, c, d, e, f = (int(v) for v in matrix)
    U = (2 * np.arange(ow, dtype=np.int64) + 1)[None, :]
    V = (2 * np.arange(oh, dtype=np.int64) + 1)[:, None]
    Nx, Ny = a * U + b * V + c, d * U + e * V + f
    if not flags & PROJECTIVE:
        return Nx, Ny
    g, h = proj_of(reserved)
    F = proj_bits(ow, oh)
    W = (1 << F) + g * (U - ow) + h * (V - oh)
    if W.min() <= 0:
        raise ValueError("positions: the denominator is not positive inside the output")
    return _scaled_quotient(Nx, W, F), _scaled_quotient(Ny, W, F)


def as_crop(it) -> Tuple[int, int, int, int, int, int]:
    """The item's (image, x, y, width, height, 0): what the plan looks at."""
    image, x, y, w, h = fields(it)[:5]
    return image, x, y, w, h, 0


def _wrong(w: int, h: int, rect, out_size, matrix, flags: int, reserved: int = 0) -> str:
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    a, b, c, d, e, f = (int(v) for v in matrix)
    if cw < 1 or rh < 1 or ow < 1 or oh < 1:
        return "zero width or height"
    if x < 0 or y < 0 or x + cw > w or y + rh > h:
        return "the rectangle leaves its image"
    if ow >= MAX_OUT or oh >= MAX_OUT:
        return "out_width or out_height from 2**20"
    if ow * oh >= MAX_AREA:
        return "out_width * out_height from 400 000 000"
    if abs(c) >= MAX_OFFSET or abs(f) >= MAX_OFFSET:
        return "|c| or |f| from 2**56"
    if any(not -2 ** 31 <= v < 2 ** 31 for v in (a, b, d, e)):
        return "a, b, d, e are 32-bit"
    if flags & ~(BORDERS | NEAREST | BICUBIC | SUPERS | VOTES | PROJECTIVE):
        return "unknown flag bit"
    if flags & NEAREST and flags & BICUBIC:
        return "NEAREST and BICUBIC together"
    if (flags & BORDERS) & ((flags & BORDERS) - 1):
        return "more than one border of REPLICATE, REFLECT, REFLECT_101 and WRAP"
    if flags & SUPERS == SUPERS:
        return "SUPER2 and SUPER4 together"
    if flags & SUPERS and flags & (NEAREST | BICUBIC):
        return "supersampling is defined for the bilinear sampling only: a SUPER flag with NEAREST or BICUBIC"
    if flags & VOTES == VOTES:
        return "VOTE2 and VOTE4 together"
    if flags & VOTES and flags & (NEAREST | BICUBIC | SUPERS):
        return "the vote is a sampling of its own: a VOTE flag with NEAREST, BICUBIC, SUPER2 or SUPER4"
    if flags & PROJECTIVE:                                              # reserved holds g and h
        if flags & (SUPERS | VOTES):
            return "the projective map is defined for the bilinear, nearest and bicubic samplings: PROJECTIVE with a SUPER or VOTE flag"
        if abs(c) >= PROJ_MAX_OFFSET or abs(f) >= PROJ_MAX_OFFSET:
            return "|c| or |f| from 2**53 with PROJECTIVE"
        g, h = proj_of(reserved)
        F = proj_bits(ow, oh)
        if (1 << F) - abs(g) * (ow - 1) - abs(h) * (oh - 1) < 1 << (F - 3):
            return "the denominator of PROJECTIVE falls below 1/8 inside the output"
        return ""
    if reserved:
        return "reserved is not 0"
    return ""


def fold(k, n: int, border: int) -> np.ndarray:
    """int64 like k: the tap indices k (any integers) on an axis of n samples folded into [0, n) under the border ``REFLECT``,
    ``REFLECT_101`` or ``WRAP``."""
    k = np.asarray(k, dtype=np.int64)
    if n < 1 or border not in (REFLECT, REFLECT_101, WRAP):
        raise ValueError("fold: n >= 1 and one of REFLECT, REFLECT_101, WRAP")
    if border == WRAP:
        return k % n                                                     # (numpy's % floors)
    if border == REFLECT:
        m = k % (2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    if n == 1:
        return np.zeros_like(k)
    m = k % (2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


def _border(k: np.ndarray, n: int, flags: int):
    """(indices inside [0, n), taken-from-R) of the tap indices k under the item's border: folded, clamped, or the fill where outside."""
    if flags & (BORDERS & ~REPLICATE):
        return fold(k, n, flags & BORDERS), np.ones(k.shape, dtype=bool)
    if flags & REPLICATE:
        return np.clip(k, 0, n - 1), np.ones(k.shape, dtype=bool)
    return np.clip(k, 0, n - 1), (k >= 0) & (k < n)


def _axis(P: np.ndarray, n: int, flags: int):
    """(indices int64[..., 2] inside [0, n), weights int64[..., 2], taken-from-R bool[..., 2]) of the positions P on an axis of n samples
    (flags: the item's, of which the border counts; a bool is taken as ``REPLICATE`` or not)."""
    p = P - ONE
    k0 = p >> 17
    fr = p & (2 * ONE - 1)
    k = np.stack([k0, k0 + 1], axis=-1)
    wgt = np.stack([2 * ONE - fr, fr], axis=-1)
    i, inside = _border(k, n, int(flags))
    return i, wgt, inside


def cubic_weights(fr) -> np.ndarray:
    """int64[..., 4]: the q of the samples k0 - 1 .. k0 + 2 for the fractions fr (0 .. 2**17 - 1); every last axis sums to 2**15."""
    fr = np.asarray(fr, dtype=np.int64)
    u = 2 * ONE
    d = np.stack([u + fr, fr, u - fr, 2 * u - fr], axis=-1)
    c = np.where(d <= u, 3 * d ** 3 - 5 * u * d ** 2 + 2 * u ** 3, -d ** 3 + 5 * u * d ** 2 - 8 * u * u * d + 4 * u ** 3)   # (c(2u) = 0)
    if not (c.sum(axis=-1) == 1 << 52).all():
        raise AssertionError("cubic_weights: the four c do not add up to 2**52")
    q = (c + (1 << 36)) >> 37
    best = np.argmax(c, axis=-1)[..., None]                              # (argmax: the lowest j of the largest c)
    np.put_along_axis(q, best, np.take_along_axis(q, best, axis=-1) + (CUBIC_ONE - q.sum(axis=-1))[..., None], axis=-1)
    if np.abs(q).sum(axis=-1).max(initial=0) > CUBIC_L1_MAX:
        raise AssertionError("cubic_weights: sum |q| above its bound")
    return q


def _cubic_axis(P: np.ndarray, n: int, flags: int):
    """(indices int64[..., 4] inside [0, n), weights int64[..., 4], taken-from-R bool[..., 4]) of the positions P on an axis of n samples
    (flags: as for ``_axis``)."""
    p = P - ONE
    k = (p >> 17)[..., None] + np.arange(-1, 3, dtype=np.int64)
    i, inside = _border(k, n, int(flags))
    return i, cubic_weights(p & (2 * ONE - 1)), inside


def _clamp(v: np.ndarray) -> np.ndarray:
    return np.minimum(np.maximum(v, 0), 255)


def cubic_reference(D: np.ndarray, rect, out_size, matrix=IDENTITY, flags: int = 0, fill: int = 0, reserved: int = 0) -> np.ndarray:
    """float64[out_height, out_width, och]: Keys' kernel (a = -1/2) at the same positions with the same border rule (``fill``, ``REPLICATE``
    or a folding border), evaluated in
    float64, PLAIN, neither rounded nor clamped (positions below 2**53 are exact there)."""
    D = np.asarray(D)
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    a, b, c, d, e, f = (int(v) for v in matrix)
    och = D.shape[2]
    R = D[y:y + rh, x:x + cw].astype(np.float64)
    F = np.array([(fill >> (8 * k)) & 255 for k in range(och)], dtype=np.float64)
    U = (2 * np.arange(ow, dtype=np.int64) + 1)[None, :]
    V = (2 * np.arange(oh, dtype=np.int64) + 1)[:, None]

    def axis(P, n):
        p = P - ONE
        k = (p >> 17)[..., None] + np.arange(-1, 3, dtype=np.int64)
        t = np.abs((p & (2 * ONE - 1)).astype(np.float64)[..., None] / (2 * ONE) - np.arange(-1, 3, dtype=np.float64))
        w = np.where(t <= 1, 1.5 * t ** 3 - 2.5 * t ** 2 + 1, np.where(t < 2, -0.5 * t ** 3 + 2.5 * t ** 2 - 4 * t + 2, 0.0))
        i, inside = _border(k, n, flags)
        return i, w, inside

    Px, Py = positions((ow, oh), matrix, flags, reserved)
    kx, wx, inx = axis(Px, cw)
    ky, wy, iny = axis(Py, rh)
    out = np.zeros((oh, ow, och), dtype=np.float64)
    for r in range(4):
        for k in range(4):
            v = np.where((iny[..., r] & inx[..., k])[..., None], R[ky[..., r], kx[..., k]], F[None, None, :])
            out += (wy[..., r] * wx[..., k])[..., None] * v
    return out


def cubic_bound() -> int:
    """The most a PLAIN byte of a ``BICUBIC`` item differs from ``round(clamp(cubic_reference))``: floor(1 + E) of the docstring."""
    e_num = 255 * 3 * (3 + 3) * (1 << 14) + 255 * 3 * 3                  # E * 2**31 with T = 4 and L = 3/2 in both axes
    return 1 + e_num // (1 << 31)


def warp(D: np.ndarray, rect: Tuple[int, int, int, int], out_size: Tuple[int, int], matrix=IDENTITY, flags: int = 0, fill: int = 0,
         mode: int = PLAIN, och: int = 0, reserved: int = 0) -> np.ndarray:
    """D uint8[h, w, 3 or 4], rect (x, y, width, height) inside it, out_size (out_width, out_height), matrix (a, b, c, d, e, f)
    -> uint8[out_height, out_width, och]; och 0 is D's own channel count; reserved: the item's, g and h under ``PROJECTIVE``.  D with 3 channels is a decode whose alpha is 255; a 4-channel
    stream decoded with och 3 under a ``VOTE`` flag is stated by its 4-channel decode as D and och = 3: its alpha votes, the output lacks it
    (``mode.mode`` likewise; every other sampling gives the bytes of the 3-channel decode either way)."""
    D = np.asarray(D)
    if D.ndim != 3 or D.shape[2] not in (3, 4) or D.dtype != np.uint8:
        raise ValueError("warp: D must be uint8[h, w, 3 or 4]")
    if mode not in (PLAIN, ALPHA_WEIGHTED):
        raise ValueError("warp: mode must be PLAIN or ALPHA_WEIGHTED")
    wrong = _wrong(D.shape[1], D.shape[0], rect, out_size, matrix, flags, reserved)
    if wrong:
        raise ValueError("warp: " + wrong)
    if not 0 <= fill < 2 ** 32:
        raise ValueError("warp: fill is 32-bit")
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    a, b, c, d, e, f = (int(v) for v in matrix)
    if och not in (0, 3, 4):
        raise ValueError("warp: och must be 3 or 4")
    och = och or D.shape[2]
    weighted = mode == ALPHA_WEIGHTED and och == 4
    R = D[y:y + rh, x:x + cw].astype(np.int64)
    if D.shape[2] == 3:
        R = np.concatenate([R, np.full((rh, cw, 1), 255, dtype=np.int64)], axis=2)
    F = np.array([(fill >> (8 * k)) & 255 for k in range(4)], dtype=np.int64)
    U = (2 * np.arange(ow, dtype=np.int64) + 1)[None, :]
    V = (2 * np.arange(oh, dtype=np.int64) + 1)[:, None]
    Pxc, Pyc = positions((ow, oh), matrix, flags, reserved)              # of the pixel's own centre: a*U + b*V + c, d*U + e*V + f without PROJECTIVE

    def select(Px, Py):
        """the one sample of NEAREST at the positions: R[Py >> 17][Px >> 17], brought inside by the border, or the fill"""
        k, ink = _border(Px >> 17, cw, flags)
        r, inr = _border(Py >> 17, rh, flags)
        return np.where((ink & inr)[..., None], R[r, k], F[None, None, :])

    if flags & NEAREST:
        return np.ascontiguousarray(select(Pxc, Pyc)[..., :och].astype(np.uint8))
    if flags & VOTES:
        L = vote_log2(flags)
        s = 1 << L
        keys = []                                                        # of every sub-sample: r << 24 | g << 16 | b << 8 | a
        for j in range(s):
            for i in range(s):
                Us, Vs = s * U + (2 * i + 1 - s), s * V + (2 * j + 1 - s)
                keys.append(_key(select(((a * Us + b * Vs) >> L) + c, ((d * Us + e * Vs) >> L) + f)))
        keys = np.stack(keys, axis=-1)                                   # int64[oh, ow, s * s]
        centre = _key(select(Pxc, Pyc))                                  # decides a tie where it is a winner; it does not vote
        count = (keys[..., :, None] == keys[..., None, :]).sum(axis=-1)
        word = (count << 33) | ((keys == centre[..., None]).astype(np.int64) << 32) | (0xFFFFFFFF - keys)   # the largest: count, centre, lowest key
        win = np.take_along_axis(keys, np.argmax(word, axis=-1)[..., None], axis=-1)[..., 0]
        out = np.stack([(win >> sh) & 255 for sh in (24, 16, 8, 0)], axis=-1)
        return np.ascontiguousarray(out[..., :och].astype(np.uint8))
    if flags & BICUBIC:
        kx, qx, inx = _cubic_axis(Pxc, cw, flags)
        ky, qy, iny = _cubic_axis(Pyc, rh, flags)
        N = np.zeros((oh, ow, 4), dtype=np.int64)
        M = np.zeros((oh, ow, 3), dtype=np.int64)
        for r in range(4):
            for k in range(4):
                v = np.where((iny[..., r] & inx[..., k])[..., None], R[ky[..., r], kx[..., k]], F[None, None, :])
                wgt = (qy[..., r] * qx[..., k])[..., None]               # signed; a sample without a weight adds nothing
                N += wgt * v                                             # below 2**40 in magnitude
                M += wgt * v[..., :3] * v[..., 3:4]                      # below 2**48
        out = _clamp((N + (1 << 29)) >> 30)
        if weighted:
            A = N[..., 3:4]
            out[..., :3] = np.where(A > 0, _clamp((M + A // 2) // np.maximum(A, 1)), out[..., :3])
        return np.ascontiguousarray(out[..., :och].astype(np.uint8))
    L = super_log2(flags)                                                # 0 without a SUPER flag: one sample, Us = U, Vs = V, no shift
    s = 1 << L
    N = np.zeros((oh, ow, 4), dtype=np.int64)
    M = np.zeros((oh, ow, 3), dtype=np.int64)
    for j in range(s):
        for i in range(s):
            Us, Vs = s * U + (2 * i + 1 - s), s * V + (2 * j + 1 - s)    # below 2**23; the sums below are under 2**55
            Px, Py = (Pxc, Pyc) if L == 0 else (((a * Us + b * Vs) >> L) + c, ((d * Us + e * Vs) >> L) + f)   # (L == 0: Us = U, Vs = V)
            kx, wx, inx = _axis(Px, cw, flags)
            ky, wy, iny = _axis(Py, rh, flags)
            for r in range(2):
                for k in range(2):
                    v = np.where((iny[..., r] & inx[..., k])[..., None], R[ky[..., r], kx[..., k]], F[None, None, :])
                    wgt = (wy[..., r] * wx[..., k])[..., None]           # at most 2**34; a sample without a weight adds nothing
                    N += wgt * v                                         # below 2**42, 2**46 over 4 x 4 sub-samples
                    M += wgt * v[..., :3] * v[..., 3:4]                  # below 2**50, 2**54
    out = (N + (1 << (33 + 2 * L))) >> (34 + 2 * L)
    if weighted:
        A = N[..., 3:4]
        out[..., :3] = np.where(A > 0, (M + A // 2) // np.maximum(A, 1), out[..., :3])
    return np.ascontiguousarray(out[..., :och].astype(np.uint8))


def _key(px: np.ndarray) -> np.ndarray:
    """int64[...]: r << 24 | g << 16 | b << 8 | a of the pixels int64[..., 4] (``mode.key``)"""
    return px[..., 0] << 24 | px[..., 1] << 16 | px[..., 2] << 8 | px[..., 3]


def vote_log2(flags: int) -> int:
    """L of the item's flags: 1 for ``VOTE2``, 2 for ``VOTE4``, 0 without; s = 1 << L nearest sub-samples along each axis of an output pixel."""
    return 2 if flags & VOTE4 else (1 if flags & VOTE2 else 0)


def vote_reference(D: np.ndarray, rect, out_size, matrix=IDENTITY, flags: int = 0, fill: int = 0, census=None, och: int = 0) -> np.ndarray:
    """uint8[out_height, out_width, och]: a ``VOTE2`` / ``VOTE4`` item by the words of the definition, pixel by pixel in Python integers
    with a ``collections.Counter`` - deliberately naive, sharing with ``warp`` only ``fold`` for the three folding borders.  census, a dict,
    counts the output pixels by how they were decided: 'unique', 'centre' (a tie the centre value wins), 'lowest' (a tie in which the centre
    value is no winner).  och as for ``warp``."""
    from collections import Counter
    D = np.asarray(D)
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    a, b, c, d, e, f = (int(v) for v in matrix)
    sch, och = D.shape[2], och or D.shape[2]
    L = vote_log2(flags)
    s = 1 << L
    border = flags & BORDERS
    F = tuple((fill >> (8 * k)) & 255 for k in range(4))

    def index(k, n):
        if border == 0:
            return k if 0 <= k < n else None
        if border == REPLICATE:
            return min(max(k, 0), n - 1)
        return int(fold(k, n, border))

    def value(Px, Py):
        k, r = index(Px >> 17, cw), index(Py >> 17, rh)
        if k is None or r is None:
            return F                                                     # the fill as given, all four bytes; nothing is read
        px = tuple(int(v) for v in D[y + r, x + k])
        return px + ((255,) if sch == 3 else ())

    out = np.zeros((oh, ow, och), dtype=np.uint8)
    for Y in range(oh):
        for X in range(ow):
            Uo, Vo = 2 * X + 1, 2 * Y + 1
            votes = Counter()
            for j in range(s):
                for i in range(s):
                    Us, Vs = s * Uo + 2 * i + 1 - s, s * Vo + 2 * j + 1 - s
                    votes[value(((a * Us + b * Vs) >> L) + c, ((d * Us + e * Vs) >> L) + f)] += 1
            top = max(votes.values())
            winners = sorted(v for v, n in votes.items() if n == top)   # (r, g, b, a) ascending: by key
            centre = value(a * Uo + b * Vo + c, d * Uo + e * Vo + f)
            win = centre if centre in winners else winners[0]
            if census is not None:
                kind = "unique" if len(winners) == 1 else ("centre" if centre in winners else "lowest")
                census[kind] = census.get(kind, 0) + 1
            out[Y, X] = win[:och]
    return out


def super_log2(flags: int) -> int:
    """L of the item's flags: 1 for ``SUPER2``, 2 for ``SUPER4``, 0 without; s = 1 << L sub-samples along each axis of an output pixel."""
    return 2 if flags & SUPER4 else (1 if flags & SUPER2 else 0)


def super_reference(D: np.ndarray, rect, out_size, matrix=IDENTITY, flags: int = 0, fill: int = 0) -> np.ndarray:
    """float64[out_height, out_width, och]: the mean of the bilinear samples at the s**2 integer positions (Px, Py) of every output pixel
    with the item's border rule (``fill``, ``REPLICATE`` or a folding border), evaluated in float64, PLAIN, not rounded (weights and values
    are exact doubles; only the sums round)."""
    D = np.asarray(D)
    x, y, cw, rh = (int(v) for v in rect)
    ow, oh = (int(v) for v in out_size)
    a, b, c, d, e, f = (int(v) for v in matrix)
    och = D.shape[2]
    R = D[y:y + rh, x:x + cw].astype(np.float64)
    F = np.array([(fill >> (8 * k)) & 255 for k in range(och)], dtype=np.float64)
    U = (2 * np.arange(ow, dtype=np.int64) + 1)[None, :]
    V = (2 * np.arange(oh, dtype=np.int64) + 1)[:, None]
    L = super_log2(flags)
    s = 1 << L
    out = np.zeros((oh, ow, och), dtype=np.float64)
    for j in range(s):
        for i in range(s):
            Us, Vs = s * U + (2 * i + 1 - s), s * V + (2 * j + 1 - s)
            kx, wx, inx = _axis(((a * Us + b * Vs) >> L) + c, cw, flags)
            ky, wy, iny = _axis(((d * Us + e * Vs) >> L) + f, rh, flags)
            for r in range(2):
                for k in range(2):
                    v = np.where((iny[..., r] & inx[..., k])[..., None], R[ky[..., r], kx[..., k]], F[None, None, :])
                    out += ((wy[..., r] / (2.0 * ONE)) * (wx[..., k] / (2.0 * ONE)))[..., None] * v
    return out / (s * s)


def size(w: int, h: int, it, och: int) -> int:
    """Bytes of the item's output for an image of w x h: out_width * out_height * och, or 0 where ``qoimi_warp_size`` returns 0 for an
    accepted descriptor."""
    _, x, y, cw, rh, ow, oh, flags, a, b, d, e, _, reserved, c, f = fields(it)
    if och not in (3, 4) or _wrong(w, h, (x, y, cw, rh), (ow, oh), (a, b, c, d, e, f), flags, reserved):
        return 0
    return ow * oh * och


def plan(descs, items, staging_bytes: int):
    """``crops.plan`` over the items' (image, x, y, width, height): (images, slots, subs, largest); ``len(subs)`` is what
    ``qoimi_warp_stats`` reports as [0] and [1], ``largest`` as [2], ``len(images)`` as [3]."""
    return crops.plan(descs, [as_crop(it) for it in items], staging_bytes)


def orient(w: int, h: int, rect: Tuple[int, int, int, int], orientation: int) -> Optional[Tuple[int, ...]]:
    """The item (image 0) that shows rect of an image of w x h in the EXIF orientation 1..8, as ``qoimi_warp_orient`` fills it; None where
    that returns an error.  1 as it is, 2 mirrored left-right, 3 turned by 180 degrees, 4 mirrored top-bottom, 5 transposed, 6 turned by 90
    degrees clockwise, 7 transposed along the other diagonal, 8 turned by 90 degrees counter-clockwise."""
    x, y, cw, rh = (int(v) for v in rect)
    if orientation not in range(1, 9) or cw < 1 or rh < 1 or x < 0 or y < 0 or x + cw > w or y + rh > h:
        return None
    transposed = orientation >= 5
    sx = -ONE if orientation in (2, 3, 7, 8) else ONE                   # the rectangle's columns run backwards
    sy = -ONE if orientation in (3, 4, 6, 7) else ONE                   # ... its rows
    c = 2 * cw * ONE if sx < 0 else 0                                   # 2 * (cw - 1 - k) + 1 = 2 * cw - (2k + 1)
    f = 2 * rh * ONE if sy < 0 else 0
    matrix = (0, sx, c, sy, 0, f) if transposed else (sx, 0, c, 0, sy, f)
    return item(0, rect, (rh, cw) if transposed else (cw, rh), matrix)


def rotation(rect_size: Tuple[int, int], out_size: Tuple[int, int], degrees: float, scale: float = 1.0) -> Tuple[int, ...]:
    """(a, b, c, d, e, f) quantised to 2**-16: the output shows the rectangle turned by `degrees` counter-clockwise about its centre and
    enlarged by `scale`, the rectangle's centre at the output's centre."""
    import math
    cw, rh = rect_size
    ow, oh = out_size
    t = math.radians(degrees)
    co, si = math.cos(t) / scale, math.sin(t) / scale
    a, b, d, e = (int(round(v * ONE)) for v in (co, -si, si, co))
    # the output's centre (U, V) = (ow, oh) in doubled coordinates goes to the rectangle's centre (cw, rh) << 16
    return (a, b, cw * ONE - a * ow - b * oh, d, e, rh * ONE - d * ow - e * oh)


def homography(rect_size: Tuple[int, int], out_size: Tuple[int, int], H):
    """((a, b, c, d, e, f), (g, h), displacement) of the ``PROJECTIVE`` item that shows the rectangle through the 3 x 3 float matrix H, which
    takes output pixel centres to source pixel centres of the rectangle: ``(k, r) = (H0 . (X, Y, 1), H1 . (X, Y, 1)) / (H2 . (X, Y, 1))``
    with pixel (0, 0)'s centre at (0, 0) on both sides.  The denominator is normalised to 1 at the output's centre - it must not vanish
    there - and everything is quantised: g and h to ``2**-F`` per doubled pixel, a, b, d, e to ``2**-16``, c and f so that the output's
    centre keeps its place to ``2**-17`` of a pixel.  displacement is the largest distance in source pixels between the real and the
    quantised map over the four corner pixels of the output: the accuracy is REPORTED, not promised, and whether the item is accepted is
    ``_wrong``'s to say (a horizon inside or near the output is not)."""
    H = np.asarray(H, dtype=np.float64)
    if H.shape != (3, 3):
        raise ValueError("homography: H is 3 x 3")
    cw, rh = rect_size
    if cw < 1 or rh < 1:
        raise ValueError("homography: an empty rectangle")
    ow, oh = (int(v) for v in out_size)
    F = proj_bits(ow, oh)
    Dc = H[2, 0] * (ow - 1) / 2 + H[2, 1] * (oh - 1) / 2 + H[2, 2]       # the denominator at the output's centre (U, V) = (ow, oh)
    if not np.isfinite(H).all() or Dc == 0:
        raise ValueError("homography: the denominator vanishes at the output's centre")
    H = H / Dc
    g, h = (int(round(float(v) * 2 ** F / 2)) for v in (H[2, 0], H[2, 1]))   # X - Xc = Uc / 2
    # the doubled position (2k + 1) * ONE = ONE * (2 * numerator + denominator) / denominator: its numerator is linear in U = 2X + 1, V = 2Y + 1
    rows = []
    for n in (H[0], H[1]):
        m = 2 * n + H[2]
        rows.append((ONE * m[0] / 2, ONE * m[1] / 2, ONE * (m[2] - m[0] / 2 - m[1] / 2)))
    (ar, br, cr), (dr, er, fr) = rows
    a, b, d, e = (int(round(v)) for v in (ar, br, dr, er))
    c = int(round(ar * ow + br * oh + cr)) - a * ow - b * oh             # the centre's numerator, where W is 2**F exactly
    f = int(round(dr * ow + er * oh + fr)) - d * ow - e * oh
    if not (-2 ** 15 <= g < 2 ** 15 and -2 ** 15 <= h < 2 ** 15) or any(not -2 ** 31 <= v < 2 ** 31 for v in (a, b, d, e)):
        raise ValueError("homography: a coefficient leaves its 16 or 32 bits")
    worst = 0.0
    for X in (0, ow - 1):
        for Y in (0, oh - 1):
            den = H[2, 0] * X + H[2, 1] * Y + H[2, 2]
            U, V = 2 * X + 1, 2 * Y + 1
            W = 2 ** F + g * (U - ow) + h * (V - oh)
            if den == 0 or W == 0:
                worst = float("inf")
                continue
            real = np.array([H[0] @ (X, Y, 1.0), H[1] @ (X, Y, 1.0)]) / den
            quant = (np.array([a * U + b * V + c, d * U + e * V + f], dtype=np.float64) * 2.0 ** F / W / ONE - 1) / 2
            worst = max(worst, float(np.hypot(*(real - quant))))
    return (a, b, c, d, e, f), (g, h), worst


def perspective(rect_size: Tuple[int, int], out_size: Tuple[int, int], corners):
    """``homography`` of the map under which the output's four corner pixels - top-left, top-right, bottom-right, bottom-left - show the four
    source points ``corners`` ((x, y) in pixel-centre coordinates of the rectangle, in that order): torchvision's ``endpoints`` with the
    output's corners as ``startpoints``."""
    ow, oh = (int(v) for v in out_size)
    if ow < 2 or oh < 2:
        raise ValueError("perspective: the output's corners must be four different pixels")
    src = np.asarray(corners, dtype=np.float64)
    if src.shape != (4, 2):
        raise ValueError("perspective: four (x, y) points")
    dst = [(0, 0), (ow - 1, 0), (ow - 1, oh - 1), (0, oh - 1)]
    A, rhs = [], []
    for (X, Y), (k, r) in zip(dst, src):
        A.append([X, Y, 1, 0, 0, 0, -k * X, -k * Y]); rhs.append(k)
        A.append([0, 0, 0, X, Y, 1, -r * X, -r * Y]); rhs.append(r)
    try:
        p = np.linalg.solve(np.array(A, dtype=np.float64), np.array(rhs, dtype=np.float64))
    except np.linalg.LinAlgError:
        raise ValueError("perspective: the four points do not define a homography")
    return homography(rect_size, out_size, np.append(p, 1.0).reshape(3, 3))


# ---------------------------------------------------------------------------------- the kernel's tiles
def tiles(ow: int, oh: int) -> int:
    """Tiles of 16 x 16 output pixels of an item."""
    return -(-ow // TILE) * -(-oh // TILE)


def place(tile: int, t: int, ow: int, oh: int) -> Optional[Tuple[int, int]]:
    """(X, Y) of work item t (0..255) of a tile, None beyond an edge of the output."""
    across = -(-ow // TILE)
    ty, tx = divmod(tile, across)
    X, Y = tx * TILE + (t & 15), ty * TILE + (t >> 4)
    return (X, Y) if X < ow and Y < oh else None
