"""``qoimi_encode_tiles`` as pure functions - the normative statement of a tile's pixels (what qoi_tile.hip gathers from the caller's images
before the encoder runs), of ``qoimi_tile_size``, of ``qoimi_tile_pyramid`` and of the staging plan (plain numpy / integer arithmetic, no GPU),
composed from the models of the serving side: ``thumbs.thumbnail`` and ``crops.crop``.

A tile is ``(image, x, y, width, height, factor, flags, reserved)`` - the fields of ``qoimi_tile`` in their order; an ``api.QoimiTile`` is taken
as well.  With S the image as ``uint8[h, w, sch]``: ``R = S[y:y+height, x:x+width]``, ``T = thumbs.thumbnail(R, factor, mode)`` at sch channels
(with 3 channels ALPHA_WEIGHTED is PLAIN), T is flipped as ``crops.crop`` flips, then converted to ``och = channels`` (or sch when channels is
0): 4 to 3 drops alpha - after the reduction -, 3 to 4 sets alpha to 255.  Stream j of the call is the reference encoder's stream of T with
the descriptor ``(tw, th, och, colorspace of the image)``.

Label maps (the mean of class 3 and class 7 is class 5) take ``mode = NEAREST`` or ``mode = MODE`` in the place of the box average - values
``qoimi_encode_tiles`` alone accepts.  R is taken at 4 bytes per pixel: a 3-channel source has alpha 255, and that alpha takes part.  The block
of output pixel (X, Y) is the box filter's, partial blocks at the right and bottom edge included: columns ``[X*f, min((X+1)*f, cw))``, nx of
them, rows ``[Y*f, min((Y+1)*f, ch))``, ny of them; its centre pixel is column ``X*f + nx // 2``, row ``Y*f + ny // 2``.

* ``NEAREST``: the output pixel is the centre pixel, byte for byte; any factor 1..64.
* ``MODE``: ``mode.vote`` over the block - whole pixels vote, all four bytes; the largest count wins; of several winners the centre pixel wins
  if it is one of them, otherwise the lowest ``r << 24 | g << 16 | b << 8 | a``.  ``factor <= MODE_MAX_FACTOR = 16``: a block holds at most
  16 x 16 pixels, the limit of ``FILTER_MODE``.

The flips and the conversion to och follow as above (4 to 3 drops alpha after the vote).  ``factor == 1`` is the rectangle itself in both
modes; a constant block gives the constant.  With f dividing cw and ch, a 4-channel source and och 4, a ``MODE`` tile is
``mode.mode(S, rect, (tw, th))`` byte for byte (for ``n_src = f * n_out`` its cells are the f-blocks and its nearest index is ``Z*f + f // 2``),
and a ``NEAREST`` tile is ``nearest.nearest``.  ``pyramid`` is unchanged: five levels (f = 1..16) can vote, levels 5 and 6 need ``NEAREST``.
The modes change no size: ``size`` and ``plan`` take no mode.

The work items of the kernel tile_select, which these two modes run in the place of tile_gather: ``select_split`` and ``select_tiles`` below.

Tensors as the source (``SRC`` and the bits beside it in a tile's flags; ``source_flags`` builds them).  The image a tile names then is a
tensor: uint8, float16, bfloat16 or float32, ``[h, w, sch]`` (HWC) or ``[sch, h, w]`` (``SRC_CHW``), tightly packed at a byte offset that is a
multiple of the element size.  ``convert`` states the byte image B it stands for: x is the element widened exactly to float32; ``UNIT``
``t = x * 255``; ``SYMMETRIC`` ``m = x * 127.5`` rounded, ``t = m + 127.5`` rounded - two roundings, the convention of ``tensors.convert``;
``BYTES`` ``t = x``; the byte is 0 if t is NaN or t <= 0, 255 if t >= 255, else t rounded to the nearest integer, ties to even; a uint8
element is the byte; alpha goes the same way.  Whether subnormals are flushed cannot change a byte: ``|t| < 0.5`` gives 0 either way.  The
tile is the tile of B without the source bits - the rectangle, the flips, och - at factor 1 only, where all four modes agree; sizes, slots and
the plan do not change.  A call is a byte call or a tensor call (``SRC`` alone marks a u8 HWC image inside a tensor call) and an image has one
format.  Two properties, asserted by tests/test_ingest_model.py: a tile with ``SRC`` alone is the tile without it, and for every byte v and
each of F32, F16 and BF16 the element ``tensors.convert`` writes for v converts back to v - scale 1/255 and bias 0 with ``UNIT``, scale 2/255
and bias -1 with ``SYMMETRIC``, scale 1 and bias 0 with ``BYTES``.  The work items of the kernel tensor_ingest, which a tensor call runs in
the place of tile_gather: ``ingest_items`` and ``ingest_tiles`` - four consecutive output pixels an item.

Label tensors as the source (``LABELS`` and the dtype bits beside it; ``label_flags`` builds them).  The image a tile names then is ONE
PLANE ``[h, w]`` of uint8, int32 or int64 class indices, tightly packed at a byte offset that is a multiple of the element size.
``labels_to_bytes`` states the byte image B it stands for: the byte b of an element v is 0 for v < 0, 255 for v > 255, else v - saturation
of the whole 32- / 64-bit value (2^32 is 255), and silent: an ignore index of -100 becomes 0 - and pixel (Y, X) of B ``uint8[h, w, 4]`` is
``(b, b, b, 255)``.  The tile is the tile of B as a 4-channel byte image without the label bits, in the call's mode: unlike a tensor tile it
may reduce, with ``NEAREST`` (factor 1..64) and ``MODE`` (factor 1..16); a label source is never averaged, so ``PLAIN`` and
``ALPHA_WEIGHTED`` take factor 1 only (``label_wrong``).  All pixels of B are grey with alpha 255, so the whole-pixel vote is the vote on b.
A call is a byte call, a tensor call or a label call, and an image has one dtype.  The descriptor's channel count only says what och is
where the call's channels is 0; ``tile`` has no descriptor, so there 0 is B's own 4.  Three properties, asserted by
tests/test_label_ingest_model.py: values in 0..255 come back from ``nearest`` of the factor-1 tile's first channel; a uint8 label tile is
the byte tile over B; with f dividing w and h a ``MODE`` label tile is ``mode.mode`` of B at ``w/f x h/f``.  The work items of the kernel
label_ingest, which a label call runs in the place of tile_gather: ``label_tiles`` - ``ingest_tiles`` at factor 1, ``select_tiles`` above.

24-bit ids (``LABELS_ID24``, bit 15, only beside ``LABELS``; ``label_flags(dtype, ids=True)``).  The plane, its dtype, its alignment and its
extent are a label tile's, but its elements are ids - an instance map, a panoptic map, superpixels - and ``label_ids_to_bytes`` states B:
the id of an element v is 0 for v < 0, 2^24 - 1 for v > 2^24 - 1, else v (``ID_MAX`` is the bound) - of the whole 32- / 64-bit value (2^32 + 5 is
2^24 - 1, not 5), silently - and pixel (Y, X) of B is ``(id & 255, (id >> 8) & 255, id >> 16, 255)``: the COCO panoptic convention
``id = R + 256 * G + 256^2 * B``.  A uint8 plane gives ``(v, 0, 0, 255)``.  Everything behind B is a label tile's.  The pixels are no longer
grey, so the vote is the whole-pixel vote as it stands: among winners without the centre pixel the lowest ``r << 24 | g << 16 | b << 8 | a``
- the order of the id's bytes from the low byte up, not the lowest id (of 256 and 1 it is 256).  An image is bytes or ids (``plan``); images
with and without the bit mix in one label call.  Three properties, asserted by tests/test_label_id_model.py: ids in 0..2^24 - 1 come back
from ``tensors.convert`` with ``tensors.HW_ID24`` of the factor-1 tile; a call without the bit gives the bytes it gave; with f dividing w and
h an ID24 ``MODE`` tile decodes to what ``mode.mode`` gives from the factor-1 tile at ``w/f x h/f``.

The plan: tile j's slot is ``tw * th * och`` rounded up to 256 plus the encode bound of its descriptor rounded up to 256; sub-batches are cut
by ``packplan.plan`` over those slots, in tile order.
"""
from typing import List, Sequence, Tuple

import numpy as np

from . import crops, mode as _mode, packplan, thumbs

FLIP_X = crops.FLIP_X
FLIP_Y = crops.FLIP_Y
PLAIN = thumbs.PLAIN
ALPHA_WEIGHTED = thumbs.ALPHA_WEIGHTED
NEAREST = 4                     # QOIMI_TILE_NEAREST (2 and 3 are not modes)
MODE = 5                        # QOIMI_TILE_MODE
MAX_FACTOR = thumbs.MAX_FACTOR
MODE_MAX_FACTOR = _mode.MAX_RATIO   # a block votes over at most 16 x 16 pixels
SRC = 16                        # QOIMI_TILE_SRC: the image is a tensor in the format the bits below give (none: u8, HWC)
SRC_CHW = 32                    # QOIMI_TILE_SRC_CHW
SRC_F16, SRC_BF16, SRC_F32 = 64, 128, 192       # QOIMI_TILE_SRC_F16 / _BF16 / _F32: the dtype field, bits 6-7
SRC_SYMMETRIC, SRC_BYTES = 256, 512             # QOIMI_TILE_SRC_SYMMETRIC / _BYTES: the range field, bits 8-9 (768 is not a range)
SRC_MASK = SRC | SRC_CHW | SRC_F32 | 768
U8, F16, BF16, F32 = 0, 1, 2, 3                 # QOIMI_TENSOR_U8 .. _F32
HWC, CHW = 0, 1
UNIT, SYMMETRIC, BYTES = 0, SRC_SYMMETRIC, SRC_BYTES
ELEM = {U8: 1, F16: 2, BF16: 2, F32: 4}
SOURCE_ARRAYS = {U8: np.uint8, F16: np.float16, BF16: np.uint16, F32: np.float32}     # (NumPy has no bfloat16: its bits)
LABELS = 2048                   # QOIMI_TILE_LABELS: the image is one plane of class indices of the dtype the bits below give (none: u8)
LABELS_I32, LABELS_I64 = 4096, 8192             # QOIMI_TILE_LABELS_I32 / _I64: the dtype field, bits 12-13 (12288 is not a dtype)
LABELS_MASK = LABELS | 12288                    # (bit 10, bit 14 and bits 16 up stay unknown; SRC_MASK is what it was)
LABELS_ID24 = 32768             # QOIMI_TILE_LABELS_ID24, bit 15: the elements are ids, spread over r, g and b (bit 14 stays unknown)
ID_MAX = (1 << 24) - 1          # the largest id
L_U8, L_I32, L_I64 = 0, 1, 2                    # the dtype field's values
LABEL_ELEM = {L_U8: 1, L_I32: 4, L_I64: 8}
LABEL_ARRAYS = {L_U8: np.uint8, L_I32: np.int32, L_I64: np.int64}
INGEST_PIXELS = 4               # output pixels of a work item of tensor_ingest
THREADS = 256                   # work items of a tile of the gather kernels
MAX_LEVELS = 7
MAX_TILE_SIDE = 1 << 24
STAGING_DEFAULT = 1 << 30
PIXEL_CAP = 400000000


def fields(t) -> Tuple[int, int, int, int, int, int, int, int]:
    """(image, x, y, width, height, factor, flags, reserved) of a tile given as such a tuple (flags and reserved may be left out: 0) or as a
    ``qoimi_tile`` structure."""
    if hasattr(t, "image"):
        return int(t.image), int(t.x), int(t.y), int(t.width), int(t.height), int(t.factor), int(t.flags), int(t.reserved)
    t = tuple(int(v) for v in t)
    if not 6 <= len(t) <= 8:
        raise ValueError("a tile is (image, x, y, width, height, factor[, flags[, reserved]])")
    return t + (0,) * (8 - len(t))


def _wh(d) -> Tuple[int, int]:
    return (int(d.width), int(d.height)) if hasattr(d, "width") else (int(d[0]), int(d[1]))


def _desc_ok(w: int, h: int, ch: int) -> bool:
    return w > 0 and h > 0 and ch in (3, 4) and h < PIXEL_CAP // w


def size(w: int, h: int, sch: int, t, channels: int = 0) -> Tuple[int, int, int]:
    """(bytes, tw, th) of a tile of an image of w x h x sch: ``tw * th * och`` with och = channels or sch - or (0, 0, 0) where
    ``qoimi_tile_size`` returns 0: a rejected image shape, an empty rectangle, one that leaves the image, a factor outside 1..64, an unknown
    flag bit, reserved != 0, channels not 0 / 3 / 4 (``image`` is not looked at)."""
    _, x, y, cw, ch, f, flags, reserved = fields(t)
    if not _desc_ok(w, h, sch) or channels not in (0, 3, 4):
        return 0, 0, 0
    if cw < 1 or ch < 1 or x < 0 or y < 0 or x + cw > w or y + ch > h or not 1 <= f <= MAX_FACTOR or (flags & ~(FLIP_X | FLIP_Y | SRC_MASK | LABELS_MASK | LABELS_ID24)) or reserved:
        return 0, 0, 0
    if source_wrong(flags, f) or label_wrong(flags, f):
        return 0, 0, 0
    tw, th = thumbs.size(cw, ch, f)
    return tw * th * (channels or sch), tw, th


# ---------------------------------------------------------------------------------- tensors as the source (QOIMI_TILE_SRC*)
def source_flags(dtype: int = U8, layout: int = HWC, range: int = UNIT) -> int:
    """The bits of ``qoimi_tile.flags`` for a tensor source: dtype ``U8`` / ``F16`` / ``BF16`` / ``F32``, layout ``HWC`` / ``CHW``, range ``UNIT``
    / ``SYMMETRIC`` / ``BYTES`` (floats only; a u8 source takes ``UNIT``, which is no bit).  Or them to a tile's flips."""
    if dtype not in (U8, F16, BF16, F32) or layout not in (HWC, CHW) or range not in (UNIT, SYMMETRIC, BYTES) or (dtype == U8 and range != UNIT):
        raise ValueError("source_flags: no such format")
    return SRC | (SRC_CHW if layout == CHW else 0) | (dtype << 6) | range


def source_format(flags: int) -> Tuple[int, int, int]:
    """(dtype, layout, range) of a tile's flags (the flips and ``SRC`` itself are not looked at)."""
    return (flags >> 6) & 3, CHW if flags & SRC_CHW else HWC, flags & (3 << 8)


def source_wrong(flags: int, factor: int = 1) -> str:
    """"" if the flags are those of a byte tile or of a tensor tile the calls accept, else what is wrong - in the order the calls look."""
    src = flags & SRC_MASK
    if not src:
        return ""
    dtype, _, rng = source_format(src)
    if not src & SRC:
        return "a SRC_* bit without SRC"
    if rng == 768:
        return "768 is not a range"
    if rng != UNIT and dtype == U8:
        return "a range with a u8 source"
    if factor != 1:
        return "a tensor source takes factor 1 only"
    return ""


def source_bytes(w: int, h: int, sch: int, flags: int) -> int:
    """Bytes the image takes behind its ``pixel_offsets`` entry: ``w * h * sch`` elements of its dtype (a byte tile: of one byte)."""
    return w * h * sch * ELEM[source_format(flags)[0]]


def widen(A: np.ndarray, dtype: int) -> np.ndarray:
    """The elements as float32, exactly: float16 and the uint16 bits of a bfloat16 widen without rounding."""
    A = np.asarray(A)
    want = SOURCE_ARRAYS[dtype]
    if A.dtype != want:
        raise ValueError("widen: the array of this dtype is " + np.dtype(want).name)
    if dtype == BF16:
        return (A.astype(np.uint32) << 16).view(np.float32)
    return A.astype(np.float32)


def to_bytes(x: np.ndarray, range: int) -> np.ndarray:
    """float32 elements -> uint8: ``t = x * 255`` (``UNIT``), ``t = x * 127.5`` and then ``+ 127.5``, each rounded to float32 (``SYMMETRIC``),
    ``t = x`` (``BYTES``); 0 where t is NaN or t <= 0, 255 where t >= 255, else t rounded to the nearest integer, ties to even."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if range == UNIT:
            t = x * np.float32(255.0)
        elif range == SYMMETRIC:
            m = x * np.float32(127.5)
            t = m + np.float32(127.5)
        elif range == BYTES:
            t = x
        else:
            raise ValueError("to_bytes: no such range")
        assert t.dtype == np.float32
        out = np.zeros(t.shape, np.uint8)
        mid = (t > 0) & (t < 255)                                      # (NaN is in neither)
        out[mid] = np.rint(t[mid]).astype(np.uint8)
        out[t >= 255] = 255
    return out


def convert(A: np.ndarray, flags: int) -> np.ndarray:
    """The tensor A - [h, w, sch] (HWC) or [sch, h, w] (CHW) of uint8 / float16 / uint16 holding bfloat16 bits / float32 - in the format the
    source bits of `flags` give -> B uint8[h, w, sch]: the byte image the tile is taken from."""
    what = source_wrong(flags)
    if what:
        raise ValueError("convert: " + what)
    dtype, layout, rng = source_format(flags)
    A = np.asarray(A)
    if A.ndim != 3 or A.shape[0 if layout == CHW else 2] not in (3, 4) or A.dtype != SOURCE_ARRAYS[dtype]:
        raise ValueError("convert: A is [h, w, 3 or 4] (HWC) or [3 or 4, h, w] (CHW) of " + np.dtype(SOURCE_ARRAYS[dtype]).name)
    if layout == CHW:
        A = np.transpose(A, (1, 2, 0))
    return np.ascontiguousarray(A if dtype == U8 else to_bytes(widen(A, dtype), rng))


def ingest_items(cw: int, ch: int) -> int:
    """Work items of a tile of a tensor call (the kernel tensor_ingest): one per ``INGEST_PIXELS`` = 4 consecutive pixels of its output."""
    return -(-cw * ch // INGEST_PIXELS)


def ingest_tiles(cw: int, ch: int) -> int:
    """Tiles of 256 work items of a tile of a tensor call."""
    return -(-ingest_items(cw, ch) // THREADS)


# ---------------------------------------------------------------------------------- label tensors as the source (QOIMI_TILE_LABELS*)
def label_flags(dtype: int = L_U8, ids: bool = False) -> int:
    """The bits of ``qoimi_tile.flags`` for a label source of dtype ``L_U8`` / ``L_I32`` / ``L_I64``, with ids its elements are 24-bit ids
    (``LABELS_ID24``).  Or them to a tile's flips."""
    if dtype not in (L_U8, L_I32, L_I64):
        raise ValueError("label_flags: no such dtype")
    return LABELS | (dtype << 12) | (LABELS_ID24 if ids else 0)


def label_dtype(flags: int) -> int:
    """The dtype field of a tile's flags (``LABELS`` itself is not looked at)."""
    return (flags >> 12) & 3


def label_wrong(flags: int, factor: int = 1, mode=None) -> str:
    """"" if the flags carry no label bit or are those of a label tile the calls accept, else what is wrong - in the order the calls look,
    behind ``source_wrong``.  mode None: ``qoimi_tile_size``, which has no mode and does not apply the averaging rule."""
    lab = flags & (LABELS_MASK | LABELS_ID24)
    if not lab:
        return ""
    if not lab & LABELS:
        return "a LABELS_* bit without LABELS"
    if label_dtype(lab) == 3:
        return "12288 is not a dtype"
    if flags & SRC_MASK:
        return "LABELS together with a SRC bit"
    if mode in (PLAIN, ALPHA_WEIGHTED) and factor != 1:
        return "a label source is never averaged"
    return ""


def label_bytes(w: int, h: int, flags: int) -> int:
    """Bytes the plane takes behind its ``pixel_offsets`` entry: ``w * h`` elements of its dtype."""
    return w * h * LABEL_ELEM[label_dtype(flags)]


def labels_to_bytes(A: np.ndarray, flags: int) -> np.ndarray:
    """The plane A ``[h, w]`` of uint8 / int32 / int64 in the dtype the label bits of `flags` give -> B ``uint8[h, w, 4]``: the byte image
    the tile is taken from.  b = 0 for v < 0, 255 for v > 255, else v - exact for the whole int64 range -; the pixel is (b, b, b, 255)."""
    what = label_wrong(flags)
    if what or not flags & LABELS:
        raise ValueError("labels_to_bytes: " + (what or "no LABELS bit"))
    A = np.asarray(A)
    want = LABEL_ARRAYS[label_dtype(flags)]
    if A.ndim != 2 or A.dtype != want:
        raise ValueError("labels_to_bytes: A is [h, w] of " + np.dtype(want).name)
    if flags & LABELS_ID24:
        return label_ids_to_bytes(A, flags)
    b = np.clip(A, 0, 255).astype(np.uint8)                            # (a clip in A's own dtype: no value is narrowed before it)
    B = np.full(A.shape + (4,), 255, dtype=np.uint8)
    B[:, :, :3] = b[:, :, None]
    return B


def label_ids_to_bytes(A: np.ndarray, flags: int) -> np.ndarray:
    """The plane A ``[h, w]`` of uint8 / int32 / int64 in the dtype the label bits of `flags` give, which carry ``LABELS_ID24`` -> B
    ``uint8[h, w, 4]``.  id = 0 for v < 0, 2^24 - 1 for v > 2^24 - 1, else v - exact for the whole int64 range -; the pixel is
    (id & 255, (id >> 8) & 255, id >> 16, 255)."""
    what = label_wrong(flags)
    if what or not flags & LABELS or not flags & LABELS_ID24:
        raise ValueError("label_ids_to_bytes: " + (what or "no LABELS or no LABELS_ID24 bit"))
    A = np.asarray(A)
    want = LABEL_ARRAYS[label_dtype(flags)]
    if A.ndim != 2 or A.dtype != want:
        raise ValueError("label_ids_to_bytes: A is [h, w] of " + np.dtype(want).name)
    ids = (A if A.dtype == np.uint8 else np.clip(A, 0, ID_MAX)).astype(np.uint32)   # (a clip in A's own dtype: no value is narrowed before it)
    B = np.full(A.shape + (4,), 255, dtype=np.uint8)
    B[:, :, 0] = ids & 255
    B[:, :, 1] = (ids >> 8) & 255
    B[:, :, 2] = ids >> 16
    return B


def label_tiles(cw: int, ch: int, f: int, och: int, mode: int) -> int:
    """Tiles of 256 work items of a tile of a label call (the kernel label_ingest): at factor 1 tensor_ingest's - four consecutive output
    pixels an item -, else tile_select's in ``NEAREST`` or ``MODE``."""
    return ingest_tiles(cw, ch) if f == 1 else select_tiles(cw, ch, f, och, mode)


def select(R: np.ndarray, f: int, mode: int) -> np.ndarray:
    """R uint8[ch, cw, sch] -> uint8[th, tw, sch]: of every f-block (the box filter's partition) the centre pixel (``NEAREST``) or the winner of
    ``mode.vote`` (``MODE``, f <= 16), taken at 4 bytes per pixel - alpha 255 behind a 3-channel R - and given back with R's channels."""
    if mode not in (NEAREST, MODE):
        raise ValueError("select: mode must be NEAREST or MODE")
    if mode == MODE and f > MODE_MAX_FACTOR:
        raise ValueError("select: factor above 16 with MODE")
    ch, cw, sch = R.shape
    tw, th = thumbs.size(cw, ch, f)
    R4 = np.full((ch, cw, 4), 255, dtype=np.uint8)
    R4[:, :, :sch] = R
    x0, y0 = np.arange(tw) * f, np.arange(th) * f
    nx, ny = np.minimum(f, cw - x0), np.minimum(f, ch - y0)
    cx, cy = x0 + nx // 2, y0 + ny // 2
    out = R4[cy[:, None], cx[None, :]].copy()                          # the centre pixels: NEAREST - and a constant block gives the constant
    if mode == MODE:
        word = R4.view(np.uint32)[:, :, 0]                             # (pixels are equal where these are)
        lo = np.minimum.reduceat(np.minimum.reduceat(word, y0, axis=0), x0, axis=1)
        hi = np.maximum.reduceat(np.maximum.reduceat(word, y0, axis=0), x0, axis=1)
        for Y, X in np.argwhere(lo != hi):                             # the blocks that hold more than one value vote
            out[Y, X] = _mode.vote(R4, (int(x0[X]), int(nx[X])), (int(y0[Y]), int(ny[Y])), (int(cx[X]), int(cy[Y])))
    return out[:, :, :sch]


def tile(S: np.ndarray, t, channels: int = 0, mode: int = PLAIN) -> np.ndarray:
    """S uint8[h, w, sch] (sch 3 or 4), t a tile of it -> uint8[th, tw, och]: the pixels stream j encodes.  A tile with ``SRC`` takes S as the
    tensor its flags describe (``convert`` states the bytes B it stands for) and is the tile of B without the source bits.  A tile with
    ``LABELS`` takes S as the plane [h, w] its flags describe (``labels_to_bytes``) and is the tile of that B in `mode`; channels 0 is B's 4."""
    _, x, y, cw, ch, f, flags, reserved = fields(t)
    if flags & (LABELS_MASK | LABELS_ID24) and not source_wrong(flags, f):
        what = label_wrong(flags, f, mode)
        if what:
            raise ValueError("tile: " + what)
        S = labels_to_bytes(S, flags)
        flags &= ~(LABELS_MASK | LABELS_ID24)
        t = (0, x, y, cw, ch, f, flags, reserved)
    if flags & SRC_MASK:
        S = convert(S, flags)                                          # (raises where the bits are no format)
        t = (0, x, y, cw, ch, f, flags & ~SRC_MASK, reserved)
        flags &= ~SRC_MASK
        if f != 1:
            raise ValueError("tile: a tensor source takes factor 1 only")
    S = np.asarray(S)
    if S.ndim != 3 or S.shape[2] not in (3, 4) or S.dtype != np.uint8:
        raise ValueError("tile: S must be uint8[h, w, 3 or 4]")
    if size(S.shape[1], S.shape[0], S.shape[2], t, channels)[0] == 0:
        raise ValueError("tile: the tile or the channel count is one qoimi_encode_tiles rejects")
    R = S[y:y + ch, x:x + cw]
    T = select(R, f, mode) if mode in (NEAREST, MODE) else thumbs.thumbnail(R, f, mode)
    T = crops.crop(T, (0, 0, T.shape[1], T.shape[0]), flags)
    och = channels or S.shape[2]
    if och == 3:
        T = T[:, :, :3]
    elif T.shape[2] == 3:
        T = np.concatenate([T, np.full(T.shape[:2] + (1,), 255, dtype=np.uint8)], axis=2)
    return np.ascontiguousarray(T)


def pyramid(w: int, h: int, tile_w: int, tile_h: int, levels: int) -> List[Tuple[int, int, int, int, int, int, int, int]]:
    """The tiles of ``qoimi_tile_pyramid`` in its order (level, row, column): level l has f = 2^l, its image of ceil(w / f) x ceil(h / f) is cut
    into tiles of tile_w x tile_h; a tile's source rectangle begins at (col * tile_w * f, row * tile_h * f) and is cut to the image."""
    if w < 1 or h < 1 or h >= PIXEL_CAP // w:
        raise ValueError("pyramid: image shape rejected")
    if not (1 <= tile_w <= MAX_TILE_SIDE and 1 <= tile_h <= MAX_TILE_SIDE):
        raise ValueError("pyramid: tile_w and tile_h must be 1..2^24")
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError("pyramid: levels must be 1..7")
    out = []
    for l in range(levels):
        f = 1 << l
        lw, lh = -(-w // f), -(-h // f)
        for row in range(-(-lh // tile_h)):
            for col in range(-(-lw // tile_w)):
                x, y = col * tile_w * f, row * tile_h * f
                out.append((0, x, y, min(tile_w * f, w - x), min(tile_h * f, h - y), f, 0, 0))
    if len(out) > 2 ** 31 - 1:
        raise ValueError("pyramid: more than 2^31 - 1 tiles")
    return out


def pyramid_index(w: int, h: int, tile_w: int, tile_h: int, levels: int) -> List[Tuple[int, int, int]]:
    """(level, row, col) of every tile of ``pyramid``, in its order."""
    return [(f.bit_length() - 1, y // (tile_h * f), x // (tile_w * f)) for (_, x, y, _, _, f, _, _) in pyramid(w, h, tile_w, tile_h, levels)]


def encode_bound(tw: int, th: int, och: int) -> int:
    """``qoimi_encode_bound`` of an accepted descriptor."""
    return tw * th * (och + 1) + 22


def plan(descs: Sequence, tiles: Sequence, channels: int, staging_bytes: int):
    """(slots, subs, largest, referenced): every tile's staging slot, (first, count) of every sub-batch as indices into ``tiles``
    (``packplan.plan`` over the slots; staging_bytes 0: 1 GiB), the bytes of the largest sub-batch - what ``qoimi_tile_stats`` reports as [2];
    ``len(subs)`` is [0] and [1] - and the number of images the tiles name: [3].  descs: ``QoiDesc`` or (w, h, channels) per image."""
    slots, named = [], set()
    srcs = [fields(t)[6] & SRC_MASK for t in tiles]
    if any(srcs) and not all(srcs):
        raise ValueError("plan: a call is a byte call or a tensor call")
    if len({(fields(t)[0], s) for t, s in zip(tiles, srcs)}) != len({fields(t)[0] for t in tiles}):
        raise ValueError("plan: an image is named with two source formats")
    labs = [fields(t)[6] & (LABELS_MASK | LABELS_ID24) for t in tiles]
    if any(labs) and not all(labs):
        raise ValueError("plan: a call is a byte call, a tensor call or a label call")
    if len({(fields(t)[0], s) for t, s in zip(tiles, labs)}) != len({fields(t)[0] for t in tiles}):
        raise ValueError("plan: an image is named with two label dtypes")
    for t in tiles:
        image = fields(t)[0]
        d = descs[image]
        w, h = _wh(d)
        sch = int(d.channels) if hasattr(d, "channels") else int(d[2])
        nbytes, tw, th = size(w, h, sch, t, channels)
        if nbytes == 0:
            raise ValueError("plan: a tile is one qoimi_encode_tiles rejects")
        slots.append(packplan.slot(nbytes) + packplan.slot(encode_bound(tw, th, channels or sch)))
        named.add(image)
    subs = packplan.plan(slots, staging_bytes if staging_bytes else STAGING_DEFAULT)      # (a slot is a multiple of 256 already)
    largest = max((sum(slots[first:first + count]) for first, count in subs), default=0)
    return slots, subs, largest, len(named)


# ---------------------------------------------------------------------------------- the work items of tile_select (NEAREST / MODE)
def select_split(f: int, mode: int) -> Tuple[int, int]:
    """(lg, c): L = 2**lg neighbouring lanes share an output pixel and hold at most c <= 4 pixels of its block each - ``mode.split(f, f, 1, 1)``
    for ``MODE``, (0, 1) for ``NEAREST`` (a lane per output pixel) and for f == 1 (the copy).  Work item ``(Y * tw + X) * L + l`` of a tile's
    entry is lane l of pixel (X, Y) of the unflipped result and holds ``mode.held(l, lg, nx, ny)`` of its block."""
    if mode not in (NEAREST, MODE) or not 1 <= f <= (MODE_MAX_FACTOR if mode == MODE else MAX_FACTOR):
        raise ValueError("select_split: a mode or factor tile_select does not run")
    return _mode.split(f, f, 1, 1) if mode == MODE else (0, 1)


def select_tiles(cw: int, ch: int, f: int, och: int, mode: int) -> int:
    """Tiles of 256 work items of a tile of the call in ``NEAREST`` or ``MODE``: f == 1 has one item per aligned 16-byte word of its
    ``cw * ch * och`` bytes (the copy of tile_gather), else ``tw * th * L`` items."""
    lg = select_split(f, mode)[0]
    if f == 1:
        return -(-(-(-cw * ch * och // 16)) // THREADS)
    tw, th = thumbs.size(cw, ch, f)
    return -(-((tw * th) << lg) // THREADS)
