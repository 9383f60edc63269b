"""Python host side of the MI355X QOI path — a ctypes binding of libqoi_mi355x.so.

Mirrors the reference's interface for this path (phoboslab/qoi ``qoi.h``):

* :func:`qoi_encode` / :func:`qoi_decode` — same argument meaning and failure
  behaviour (``None`` where the C functions return ``NULL``) as ``qoi.h:278`` /
  ``qoi.h:289``; :class:`QoiDesc` is ``qoi_desc`` (``qoi.h:236-241``).
* :class:`Context` — the additive device-resident batch API (``qoimi_*``), taking
  raw device pointers (e.g. ``torch.Tensor.data_ptr()``) and a HIP stream handle.

There is no CPU fallback here: if the shared library or the GPU is missing the
calls raise / return ``None`` exactly as the C-ABI does.  torch is NOT imported by
this module; bench.py and the tests use it only for device memory and streams.
"""
from __future__ import annotations

import ctypes
import os
import types
from typing import List, Optional, Sequence, Tuple

import numpy as np

QOI_SRGB = 0
QOI_LINEAR = 1

_HERE = os.path.dirname(os.path.abspath(__file__))
# (tests and measurement tools that want another build of the library - the test flavour, an experimental build - set this before
# the first call: tests/libsel.py; nothing in the environment changes it)
LIB_PATH = os.path.join(_HERE, "lib", "libqoi_mi355x.so")

from .abi import (PROTOTYPES, ImageDiff, QoiDesc, QoimiBand, QoimiBandInfo, QoimiCrop, QoimiPixelStat, QoimiResize,  # noqa: F401
                  QoimiSeekPoint, QoimiTensorFormat, QoimiTile, QoimiWarp, StreamInfo)

# every function include/qoi_mi355x.h declares, in its order (Part 1: the drop-in symbols of qoi.h:252,265,278,289; Part 2: additive)
EXPORTS = tuple(PROTOTYPES)


class QoiError(RuntimeError):
    pass


_lib = None


def load_library() -> ctypes.CDLL:
    """Load libqoi_mi355x.so (built in-tree by ``__graft_entry__.build()``); raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QoiError(f"{LIB_PATH} not built - run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _libc_free(p: int) -> None:
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    libc.free.restype = None
    libc.free(p)


def last_error() -> str:
    return load_library().qoimi_last_error().decode()


def _range(ctype) -> Tuple[int, int]:
    """[lo, hi) of the ctypes integer type ctype."""
    bits = 8 * ctypes.sizeof(ctype)
    return (-2 ** (bits - 1), 2 ** (bits - 1)) if ctype(-1).value < 0 else (0, 2 ** bits)


def _fits(ctype, v) -> bool:
    lo, hi = _range(ctype)
    return lo <= v < hi


def _ptr(array: np.ndarray, ctype):
    """A numpy array's memory as a pointer to ctype; the pointer keeps the array alive."""
    return array.ctypes.data_as(ctypes.POINTER(ctype))


# item structure -> (shortest and longest tuple taken for one, what the messages call it, what a malformed one is told)
_ITEMS = {QoimiCrop: (6, 6, "crop", "a {} is not six unsigned 32-bit fields"),
          QoimiTile: (6, 8, "tile", "a {} is (image, x, y, width, height, factor[, flags[, reserved]]) of unsigned 32-bit values"),
          QoimiResize: (8, 8, "item", "an {} is not eight unsigned 32-bit fields"),
          QoimiWarp: (16, 16, "item", "an {} is not the sixteen fields of a qoimi_warp"),
          QoimiBand: (3, 3, "band", "a {} is not three unsigned 32-bit fields")}


def _item_array(cls, items, shortest: int, longest: int):
    """items as an array of the structure cls: a sequence of such structures or of tuples of its first `shortest` to `longest` fields
    (the fields behind a tuple's, and behind the first `longest` of a structure, are 0); None if a tuple has another length or a value
    does not fit its field's type."""
    fields = cls._fields_[:longest]
    ranges = [_range(t) for _, t in fields]
    rows = [tuple(int(getattr(it, f)) for f, _ in fields) if isinstance(it, cls) else tuple(int(v) for v in it) for it in items]
    if any(not shortest <= len(r) <= longest or any(not lo <= v < hi for (lo, hi), v in zip(ranges, r)) for r in rows):
        return None
    return (cls * len(rows))(*[cls(*r) for r in rows])


def _desc(width: int, height: int, channels_in: int) -> Optional[QoiDesc]:
    """The descriptor of an image of width x height x channels_in, or None where a value is out of range for its field."""
    if not (_fits(ctypes.c_uint, width) and _fits(ctypes.c_uint, height) and _fits(ctypes.c_ubyte, channels_in)):
        return None
    return QoiDesc(width, height, channels_in, 0)


def _size_args(cls, width: int, height: int, channels_in: int, item):
    """What a ``qoimi_*_size`` function of an item begins with - the image's descriptor and the item as the structure cls - or None where
    either is out of range."""
    arr, desc = _item_array(cls, [item], *_ITEMS[cls][:2]), _desc(width, height, channels_in)
    return None if arr is None or desc is None else (ctypes.byref(desc), arr)


def encode_bound(width: int, height: int, channels: int) -> int:
    return int(load_library().qoimi_encode_bound(ctypes.byref(QoiDesc(width, height, channels, 0))))


def thumbnail_size(width: int, height: int, channels_in: int, factor: int, channels: int) -> Tuple[int, int, int]:
    """``qoimi_thumbnail_size`` for an image of width x height x channels_in: (bytes, tw, th) of its thumbnail at `factor` with `channels`
    (3 or 4) bytes per pixel; (0, 0, 0) where the C function returns 0."""
    desc = _desc(width, height, channels_in)
    if desc is None or not _fits(ctypes.c_uint, factor):
        return 0, 0, 0
    tw, th = ctypes.c_uint(0), ctypes.c_uint(0)
    n = int(load_library().qoimi_thumbnail_size(ctypes.byref(desc), factor, channels, ctypes.byref(tw), ctypes.byref(th)))
    return n, tw.value, th.value


def crop_size(width: int, height: int, channels_in: int, crop, channels: int) -> int:
    """``qoimi_crop_size`` for an image of width x height x channels_in: the bytes of the output of `crop` (a ``QoimiCrop`` or an (image, x, y,
    width, height, flags) tuple) with `channels` (3 or 4) bytes per pixel; 0 where the C function returns 0."""
    args = _size_args(QoimiCrop, width, height, channels_in, crop)
    return int(load_library().qoimi_crop_size(*args, channels)) if args else 0


def tile_size(width: int, height: int, channels_in: int, tile, channels: int = 0):
    """``qoimi_tile_size`` for an image of width x height x channels_in: (bytes, tw, th) of the pixels of `tile` (a ``QoimiTile`` or an
    (image, x, y, width, height, factor[, flags[, reserved]]) tuple) at `channels` (0: channels_in) bytes per pixel; (0, 0, 0) where the C
    function returns 0."""
    args = _size_args(QoimiTile, width, height, channels_in, tile)
    if args is None:
        return 0, 0, 0
    tw, th = ctypes.c_uint(0), ctypes.c_uint(0)
    n = int(load_library().qoimi_tile_size(*args, channels, ctypes.byref(tw), ctypes.byref(th)))
    return n, tw.value, th.value


def tile_pyramid(width: int, height: int, channels_in: int, tile_w: int, tile_h: int, levels: int):
    """``qoimi_tile_pyramid``: the tiles of a pyramid of `levels` levels over one image as a list of ``QoimiTile`` (image 0), in the order
    level, row, column; ``tiles.pyramid`` states them.  Raises ``QoiError`` where the C function returns QOIMI_E_ARG."""
    ok = all(0 <= int(v) < 2 ** 32 for v in (width, height, tile_w, tile_h, levels)) and 0 <= channels_in < 256
    lib = load_library()
    desc = QoiDesc(width, height, channels_in, 0) if ok else QoiDesc(0, 0, 0, 0)
    n = lib.qoimi_tile_pyramid(ctypes.byref(desc), tile_w if ok else 0, tile_h if ok else 0, levels if ok else 0, None, 0)
    if n < 0:
        raise QoiError("qoimi_tile_pyramid: " + last_error())
    arr = (QoimiTile * n)()
    if lib.qoimi_tile_pyramid(ctypes.byref(desc), tile_w, tile_h, levels, arr, n) != n:
        raise QoiError("qoimi_tile_pyramid: " + last_error())
    return list(arr)


def resize_size(width: int, height: int, channels_in: int, item, channels: int) -> int:
    """``qoimi_resize_size`` for an image of width x height x channels_in: the bytes of the output of `item` (a ``QoimiResize`` or an (image,
    x, y, width, height, out_width, out_height, flags) tuple) with `channels` (3 or 4) bytes per pixel; 0 where the C function returns 0."""
    args = _size_args(QoimiResize, width, height, channels_in, item)
    return int(load_library().qoimi_resize_size(*args, channels)) if args else 0


def bilinear_size(width: int, height: int, channels_in: int, item, channels: int) -> int:
    """``qoimi_bilinear_size`` for an image of width x height x channels_in: the bytes of the output of `item` (as for ``resize_size``) with
    `channels` (3 or 4) bytes per pixel; 0 where the C function returns 0."""
    args = _size_args(QoimiResize, width, height, channels_in, item)
    return int(load_library().qoimi_bilinear_size(*args, channels)) if args else 0


def warp_size(width: int, height: int, channels_in: int, item, channels: int) -> int:
    """``qoimi_warp_size`` for an image of width x height x channels_in: the bytes of the output of `item` (a ``QoimiWarp`` or the tuple of
    ``warp.fields``) with `channels` (3 or 4) bytes per pixel; 0 where the C function returns 0."""
    args = _size_args(QoimiWarp, width, height, channels_in, item)
    return int(load_library().qoimi_warp_size(*args, channels)) if args else 0


def tensor_format(f) -> "QoimiTensorFormat":
    """f as a ``QoimiTensorFormat``: such a structure, or the (dtype, layout, scale[4], bias[4]) of ``tensors.fmt``."""
    if isinstance(f, QoimiTensorFormat):
        return f
    dtype, layout, scale, bias = f
    if not (0 <= int(dtype) < 2 ** 32 and 0 <= int(layout) < 2 ** 32 and len(scale) == 4 and len(bias) == 4):
        raise QoiError("tensor_format: (dtype, layout, scale[4], bias[4])")
    return QoimiTensorFormat(int(dtype), int(layout), (ctypes.c_float * 4)(*[float(v) for v in scale]), (ctypes.c_float * 4)(*[float(v) for v in bias]))


def tensor_size(width: int, height: int, channels_in: int, item, filter: int, channels: int, f) -> int:
    """``qoimi_tensor_size`` for an image of width x height x channels_in: the bytes of the output of `item` (as for ``resize_size``) under
    `filter` (``tensors.FILTER_AREA`` / ``FILTER_BILINEAR`` / ``FILTER_BICUBIC`` / ``FILTER_LANCZOS`` / ``FILTER_NEAREST`` / ``FILTER_MODE``) with `channels` (3 or 4) elements per pixel
    (``tensors.HW``: one) in the format f; 0 where the C
    function returns 0."""
    args = _size_args(QoimiResize, width, height, channels_in, item)
    return int(load_library().qoimi_tensor_size(*args, filter, channels, ctypes.byref(tensor_format(f)))) if args else 0


def warp_tensor_size(width: int, height: int, channels_in: int, item, channels: int, f) -> int:
    """``qoimi_warp_tensor_size``: as ``tensor_size`` for an item of ``decode_warped_tensors`` (a ``QoimiWarp`` or the tuple of ``warp.fields``)."""
    args = _size_args(QoimiWarp, width, height, channels_in, item)
    return int(load_library().qoimi_warp_tensor_size(*args, channels, ctypes.byref(tensor_format(f)))) if args else 0


def warp_orient(width: int, height: int, channels_in: int, rect, orientation: int) -> Optional["QoimiWarp"]:
    """``qoimi_warp_orient`` for an image of width x height x channels_in: the item (image 0) that shows rect (x, y, width, height) in the
    EXIF orientation 1..8; None where the C function returns an error."""
    desc = _desc(width, height, channels_in)
    if desc is None or not (all(_fits(ctypes.c_uint, int(v)) for v in rect) and _fits(ctypes.c_int, orientation)):
        return None
    out = QoimiWarp()
    x, y, w, h = (int(v) for v in rect)
    rc = load_library().qoimi_warp_orient(ctypes.byref(desc), x, y, w, h, orientation, ctypes.byref(out))
    return out if rc == 0 else None


def seek_points(width: int, height: int, channels_in: int, interval_rows: int) -> int:
    """``qoimi_seek_points`` for an image of width x height x channels_in: ceil(height / interval_rows) - 1, or -1 where the C function
    returns -1 (a rejected descriptor, interval_rows == 0, interval_rows * width < 128)."""
    desc = _desc(width, height, channels_in)
    if desc is None or not _fits(ctypes.c_uint, interval_rows):
        return -1
    return int(load_library().qoimi_seek_points(ctypes.byref(desc), interval_rows))


def _point_array(points):
    """An index as a ``QoimiSeekPoint`` array and its length: such an array, or a numpy array of ``seekindex.POINT_DTYPE`` (copied)."""
    if isinstance(points, ctypes.Array):
        return points, len(points)
    from .seekindex import POINT_DTYPE
    a = np.ascontiguousarray(points, dtype=POINT_DTYPE).reshape(-1)
    arr = (QoimiSeekPoint * max(a.size, 1))()
    ctypes.memmove(arr, a.ctypes.data, a.nbytes)
    return arr, a.size


def band_plan(desc: QoiDesc, size: int, interval_rows: int, points, first_row: int, rows: int) -> Optional[QoimiBandInfo]:
    """``qoimi_band_plan``: what the band stream of rows [first_row, first_row + rows) of an image will be, from the image's points (a
    ``QoimiSeekPoint`` array or a numpy array of ``seekindex.POINT_DTYPE``) alone; None where the C function returns QOIMI_E_ARG."""
    if not all(0 <= int(v) < 2 ** 32 for v in (interval_rows, first_row, rows)) or not -2 ** 31 <= int(size) < 2 ** 31:
        return None
    arr, _ = _point_array(points)
    out = QoimiBandInfo()
    rc = load_library().qoimi_band_plan(ctypes.byref(desc), int(size), int(interval_rows), arr, ctypes.byref(QoimiBand(0, int(first_row), int(rows), 0)), ctypes.byref(out))
    return out if rc == 0 else None


# ----------------------------------------------------------------------------------
# drop-in functions on host memory
# ----------------------------------------------------------------------------------
def qoi_encode(data, desc: QoiDesc) -> Optional[bytes]:
    """``qoi_encode`` (qoi.h:278): raw RGB/RGBA bytes + desc -> QOI stream, ``None`` on failure."""
    lib = load_library()
    arr = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray))
                               else np.asarray(data, dtype=np.uint8))
    # the C function cannot know how long `data` is (qoi.h:278 trusts width*height*channels); this wrapper can: a short
    # buffer would make the copy engine read past the allocation
    if _desc_plausible(desc) and arr.size < desc.width * desc.height * desc.channels:
        return None
    n = ctypes.c_int(0)
    p = lib.qoi_encode(arr.ctypes.data, ctypes.byref(desc), ctypes.byref(n))
    if not p:
        return None
    try:
        return ctypes.string_at(p, n.value)
    finally:
        _libc_free(p)


def _desc_plausible(desc: QoiDesc) -> bool:
    """qoi.h:364-372's rules - only where they hold does width*height*channels say how many bytes the codec will read."""
    return (desc.width > 0 and desc.height > 0 and desc.channels in (3, 4) and desc.colorspace <= 1
            and desc.height < 400000000 // desc.width)


def qoi_decode(data: bytes, channels: int = 0, size: Optional[int] = None
               ) -> Tuple[Optional[np.ndarray], QoiDesc]:
    """``qoi_decode`` (qoi.h:289): QOI stream -> (pixels uint8[w*h*channels] or ``None``, desc)."""
    lib = load_library()
    buf = (ctypes.c_ubyte * max(len(data), 1)).from_buffer_copy(bytes(data).ljust(1, b"\0"))
    desc = QoiDesc()
    p = lib.qoi_decode(ctypes.addressof(buf), len(data) if size is None else size, ctypes.byref(desc), channels)
    if not p:
        return None, desc
    try:
        och = channels if channels else desc.channels
        return np.frombuffer(ctypes.string_at(p, desc.width * desc.height * och), dtype=np.uint8).copy(), desc
    finally:
        _libc_free(p)


def qoi_write(filename: str, data, desc: QoiDesc) -> int:
    """``qoi_write`` (qoi.h:252): returns bytes written, 0 on failure."""
    arr = np.ascontiguousarray(np.asarray(data, dtype=np.uint8))
    if _desc_plausible(desc) and arr.size < desc.width * desc.height * desc.channels:
        return 0                                     # short pixel buffer: as a failed qoi_write (qoi.h:259-263)
    return int(load_library().qoi_write(filename.encode(), arr.ctypes.data, ctypes.byref(desc)))


def qoi_read(filename: str, channels: int = 0) -> Tuple[Optional[np.ndarray], QoiDesc]:
    """``qoi_read`` (qoi.h:265)."""
    lib = load_library()
    desc = QoiDesc()
    p = lib.qoi_read(filename.encode(), ctypes.byref(desc), channels)
    if not p:
        return None, desc
    try:
        och = channels if channels else desc.channels
        return np.frombuffer(ctypes.string_at(p, desc.width * desc.height * och), dtype=np.uint8).copy(), desc
    finally:
        _libc_free(p)


# ----------------------------------------------------------------------------------
# device-resident batch API
# ----------------------------------------------------------------------------------
# the C element type of a per-image sequence, by the name the marshaller is given it under; every other one is a byte offset (size_t)
_ELEMENT = {"sizes": ctypes.c_int, "interval_rows": ctypes.c_uint, "factors": ctypes.c_uint}


class Context:
    """One GPU + workspace (``qoimi_ctx``).  Pointers are raw device addresses (ints)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        h = ctypes.c_void_p()
        rc = self._lib.qoimi_ctx_create(device, ctypes.byref(h))
        if rc != 0:
            raise QoiError(f"qoimi_ctx_create({device}) failed ({rc}): {last_error()}")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.qoimi_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise QoiError(f"{what} failed ({rc}): {last_error()}")

    # ---- marshalling: what every method below makes of its sequences --------------------------------------------------------------
    def _per_image(self, what: str, each: str, n: int, **sequences) -> dict:
        """The sequences of the call `what` that hold one value per image (for output offsets: per item), checked: each has n values,
        or the call raises "<what>: one <each>"; an int given as ``interval_rows`` or ``factors`` stands for n of it."""
        for key in ("interval_rows", "factors"):
            if isinstance(sequences.get(key), (int, np.integer)):
                sequences[key] = [int(sequences[key])] * n
        if any(len(s) != n for s in sequences.values()):
            raise QoiError(f"{what}: one {each}")
        return sequences

    def _pointers(self, sequences: dict, wraps: bool = False) -> types.SimpleNamespace:
        """Checked sequences as the C call takes them, under their names: ``descs`` as a ``qoi_desc`` array, every other one as a pointer to
        ``_ELEMENT``'s type that keeps its memory alive.  wraps: converted through ctypes, where a value outside the type wraps; else
        through numpy, which raises - every call keeps the conversion it has always had."""
        m = types.SimpleNamespace()
        for key, seq in sequences.items():
            ctype = _ELEMENT.get(key, ctypes.c_size_t)
            if key == "descs":
                value = (QoiDesc * len(seq))(*seq)
            elif wraps:
                value = (ctype * len(seq))(*[int(x) for x in seq])
            else:
                value = _ptr(np.ascontiguousarray(seq, dtype=np.dtype(ctype)), ctype)
            setattr(m, key, value)
        return m

    def _marshal(self, what: str, each: str, n: int, wraps: bool = False, **sequences) -> types.SimpleNamespace:
        return self._pointers(self._per_image(what, each, n, **sequences), wraps)

    def _gather_args(self, what: str, cls, items, stream_offsets, sizes, descs, out_offsets=None, index=None, noun: Optional[str] = None,
                     each: Optional[str] = None) -> types.SimpleNamespace:
        """What a call over items (of the structure cls, called ``noun`` in messages) of a pack makes of its sequences: n, stream_offsets,
        sizes, descs, items, out_offsets (where given) and index - empty, or for index = (interval_rows, points, point_firsts) the three
        trailing arguments of an indexed call.  each: one message for a wrong length among the pack's and the index's sequences."""
        shortest, longest, default, malformed = _ITEMS[cls]
        noun, n = noun or default, len(sizes)
        pack = dict(stream_offsets=stream_offsets, sizes=sizes, descs=descs)
        extra = dict(interval_rows=index[0], point_firsts=index[2]) if index else {}
        if each:
            pack, extra = self._per_image(what, each, n, **pack, **extra), {}
        else:
            pack = self._per_image(what, "stream offset, size and descriptor per image", n, **pack)
        if out_offsets is not None:
            pack.update(self._per_image(what, "output offset per " + noun, len(items), out_offsets=out_offsets))
        arr = _item_array(cls, items, shortest, longest)
        if arr is None:
            raise QoiError(what + ": " + malformed.format(noun))
        m = self._pointers(pack)
        if extra:
            vars(m).update(vars(self._marshal(what, "interval and first point per image", n, **extra)))
        m.n, m.items = n, arr
        m.index = (m.interval_rows, _point_array(index[1])[0], m.point_firsts) if index else ()
        return m

    def _seek_index_room(self, what: str, descs, interval_rows):
        """(points, point_firsts, pointer to the points' memory) for the seek index of images of descs at interval_rows (one per image)."""
        from .seekindex import POINT_DTYPE
        counts = [seek_points(d.width, d.height, d.channels, int(k)) for d, k in zip(descs, interval_rows)]
        if any(k < 0 for k in counts):
            raise QoiError(what + ": a rejected descriptor or interval_rows * width < 128")
        firsts = [int(x) for x in np.cumsum([0] + counts[:-1])]
        points = np.zeros(sum(counts), dtype=POINT_DTYPE)
        return points, firsts, _ptr(points if points.size else np.zeros(1, dtype=POINT_DTYPE), QoimiSeekPoint)

    def _four_counters(self, name: str) -> Tuple[int, int, int, int]:
        """The four counters the function ``qoimi_<name>`` writes for this context."""
        out = (ctypes.c_longlong * 4)()
        getattr(self._lib, "qoimi_" + name)(self._h, out)
        return tuple(int(x) for x in out)

    # ---- encode ------------------------------------------------------------------------------------------------------------------
    def encode_batch(self, d_pixels: int, pixel_stride: int, desc: QoiDesc, n_images: int,
                     d_streams: int, stream_stride: int, d_stream_len: int, stream: int = 0) -> None:
        self._check(self._lib.qoimi_encode_batch(self._h, d_pixels, pixel_stride, ctypes.byref(desc), n_images,
                                                 d_streams, stream_stride, d_stream_len, stream), "qoimi_encode_batch")

    def encode_images(self, d_pixels: int, pixel_offsets: Sequence[int], descs: Sequence[QoiDesc], d_streams: int,
                      stream_offsets: Sequence[int], d_stream_len: int, stream: int = 0) -> None:
        """Images of different shapes / channel counts in one call (``qoimi_encode_images``)."""
        m = self._marshal("encode_images", "pixel offset and one stream offset per descriptor", len(descs), wraps=True,
                          pixel_offsets=pixel_offsets, descs=descs, stream_offsets=stream_offsets)
        self._check(self._lib.qoimi_encode_images(self._h, d_pixels, m.pixel_offsets, m.descs, len(descs), d_streams, m.stream_offsets, d_stream_len, stream),
                    "qoimi_encode_images")

    def encode_status(self, stream: int = 0) -> None:
        self._check(self._lib.qoimi_encode_status(self._h, stream), "qoimi_encode_status")

    def encode_suspect_calls(self) -> int:
        """Encode calls of this context made with the exchange probe since the last passed LDS-order check when a repeat failed (0: never)."""
        return int(self._lib.qoimi_encode_suspect_calls(self._h))

    def set_encode_small_call_order(self, by_workgroup_index: bool) -> None:
        """Calls of fewer than 8 images: units by ticket (default, safe on a shared device) or by workgroup index (4 us less per 4K
        frame; then ``encode_status`` must be called before the streams are read)."""
        self._check(self._lib.qoimi_set_encode_small_call_order(self._h, 1 if by_workgroup_index else 0), "qoimi_set_encode_small_call_order")

    def encode_retries(self) -> int:
        """Calls ``encode_status`` encoded again order-free because a placement wait had given up (0: never)."""
        return int(self._lib.qoimi_encode_retries(self._h))

    def pack_streams(self, d_streams: int, stream_stride: int, d_stream_len: int, n_streams: int, align: int,
                     d_packed: int, packed_capacity: int, d_packed_off: int, stream: int = 0) -> None:
        """Strided streams -> back to back at d_packed; d_packed_off: device uint64[n_streams + 1] (``qoimi_pack_streams``, asynchronous)."""
        self._check(self._lib.qoimi_pack_streams(self._h, d_streams, stream_stride, d_stream_len, n_streams, align,
                                                 d_packed, packed_capacity, d_packed_off, stream), "qoimi_pack_streams")

    @staticmethod
    def _pack_tables(n: int):
        """The two host tables a packing call fills - offsets uint64[n + 1], sizes int32[n] - and the pointers to them."""
        off, sizes = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.intc)
        return off, sizes, (_ptr(off, ctypes.c_ulonglong), _ptr(sizes, ctypes.c_int))

    def encode_packed(self, d_pixels: int, pixel_stride: int, desc: QoiDesc, n_images: int, align: int, d_packed: int, packed_capacity: int,
                      d_packed_off: int, d_stream_len: int, staging_bytes: int = 0, stream: int = 0):
        """Pixels -> pack in one call through bounded staging (``qoimi_encode_packed``, synchronous): (offsets uint64[n + 1], sizes
        int32[n]) as numpy arrays - offsets[:n] and sizes are what ``read_descs`` / ``decode_images`` / ``inspect_streams`` take,
        offsets[n] the bytes the pack needs (larger than packed_capacity: the streams that did not fit wholly are absent)."""
        off, sizes, tables = self._pack_tables(n_images)
        self._check(self._lib.qoimi_encode_packed(self._h, d_pixels, pixel_stride, ctypes.byref(desc), n_images, align, d_packed, packed_capacity,
                                                  d_packed_off, d_stream_len, staging_bytes, *tables, stream), "qoimi_encode_packed")
        return off, sizes

    def encode_images_packed(self, d_pixels: int, pixel_offsets: Sequence[int], descs: Sequence[QoiDesc], align: int, d_packed: int,
                             packed_capacity: int, d_packed_off: int, d_stream_len: int, staging_bytes: int = 0, stream: int = 0):
        """The same for images of different shapes / channel counts (``qoimi_encode_images_packed``)."""
        n = len(descs)
        m = self._marshal("encode_images_packed", "pixel offset per descriptor", n, wraps=True, pixel_offsets=pixel_offsets, descs=descs)
        off, sizes, tables = self._pack_tables(n)
        self._check(self._lib.qoimi_encode_images_packed(self._h, d_pixels, m.pixel_offsets, m.descs, n, align, d_packed, packed_capacity,
                                                         d_packed_off, d_stream_len, staging_bytes, *tables, stream), "qoimi_encode_images_packed")
        return off, sizes

    def encode_tiles(self, d_pixels: int, pixel_offsets: Sequence[int], descs: Sequence[QoiDesc], channels: int, tiles, mode: int, align: int,
                     d_packed: int, packed_capacity: int, d_packed_off: int, d_stream_len: int, staging_bytes: int = 0, stream: int = 0):
        """Tiles and pyramid levels of device images -> pack in one call through bounded staging (``qoimi_encode_tiles``, synchronous):
        (offsets uint64[n + 1], sizes int32[n], tile descriptors) - what ``decode_images`` and the gather calls take to serve the pack.
        tiles: ``QoimiTile`` structures or (image, x, y, width, height, factor[, flags]) tuples; mode: ``tiles.PLAIN`` /
        ``tiles.ALPHA_WEIGHTED`` (the box average) or, for label maps, ``tiles.NEAREST`` (the centre pixel of every block) / ``tiles.MODE`` (the
        majority vote of ``FILTER_MODE`` over every block; factor <= 16); channels 0: every tile keeps its image's channel count;
        ``qoi_amd/tiles.py: tile`` states the pixels.  With ``tiles.source_flags(dtype, layout, range)`` in every tile's flags the images are
        tensors - u8 / f16 / bf16 / f32, HWC or CHW, factor 1 - converted on the way in (``tiles.convert``); pixel_offsets stay byte offsets
        (``tiles.source_bytes`` an image; d_pixels is an address: no length of it is looked at here).  With ``tiles.label_flags(dtype)`` in
        every tile's flags the images are one-plane u8 / int32 / int64 label maps (``tiles.labels_to_bytes``; ``tiles.label_bytes`` an
        image), saturated to 0..255 silently; they reduce with ``tiles.NEAREST`` and ``tiles.MODE`` and are never averaged.  With
        ``tiles.label_flags(dtype, ids=True)`` (``tiles.LABELS_ID24``) the elements are 24-bit ids, saturated to 0..2^24 - 1 and spread over
        r, g and b (``tiles.label_ids_to_bytes``); ``tensors.HW_ID24`` puts them together again."""
        n_images = len(descs)
        seqs = self._per_image("encode_tiles", "pixel offset per descriptor", n_images, pixel_offsets=pixel_offsets, descs=descs)
        shortest, longest, noun, malformed = _ITEMS[QoimiTile]
        arr = _item_array(QoimiTile, tiles, shortest, longest)
        if arr is None:
            raise QoiError("encode_tiles: " + malformed.format(noun))
        m, n = self._pointers(seqs, wraps=True), len(arr)
        off, sizes, tables = self._pack_tables(n)
        tds = (QoiDesc * max(n, 1))()
        self._check(self._lib.qoimi_encode_tiles(self._h, d_pixels, m.pixel_offsets, m.descs, n_images, channels, arr, n, mode, align,
                                                 d_packed, packed_capacity, d_packed_off, d_stream_len, staging_bytes, *tables, tds, stream), "qoimi_encode_tiles")
        return off, sizes, list(tds)[:n]

    def verify_images(self, d_pixels: int, pixel_offsets: Sequence[int], descs: Sequence[QoiDesc], d_streams: int,
                      stream_offsets: Sequence[int], sizes: Sequence[int], staging_bytes: int = 0, stream: int = 0):
        """Do the streams decode back to exactly these pixels (``qoimi_verify_images``, synchronous, through bounded staging)?
        (diffs, first_diff) as ``compare_images`` gives them; a stream whose header does not match its descriptor is flagged
        ``imagediff.DIFF_HEADER`` and not decoded."""
        from .imagediff import DIFF_DTYPE
        n = len(descs)
        m = self._marshal("verify_images", "pixel offset, stream offset and size per descriptor", n,
                          pixel_offsets=pixel_offsets, stream_offsets=stream_offsets, sizes=sizes, descs=descs)
        diffs, first = np.zeros(n, dtype=DIFF_DTYPE), ctypes.c_int(-1)
        self._check(self._lib.qoimi_verify_images(self._h, d_pixels, m.pixel_offsets, m.descs, n, d_streams, m.stream_offsets, m.sizes, staging_bytes,
                                                  _ptr(diffs, ImageDiff), ctypes.byref(first), stream), "qoimi_verify_images")
        return diffs, first.value

    def compare_images(self, d_a: int, a_offsets: Sequence[int], a_channels: int, d_b: int, b_offsets: Sequence[int], b_channels: int,
                       descs: Sequence[QoiDesc], stream: int = 0):
        """Two sets of device images, pixel by pixel (``qoimi_compare_images``): (diffs, first_diff) - diffs is a numpy array of
        ``imagediff.DIFF_DTYPE``, first_diff the lowest index with flags != 0 or -1, as the C call gives it.  a_channels / b_channels: bytes per pixel of a side,
        0 for each image's ``descs[i].channels``."""
        from .imagediff import DIFF_DTYPE
        n = len(descs)
        m = self._marshal("compare_images", "offset per side and descriptor", n, a_offsets=a_offsets, b_offsets=b_offsets, descs=descs)
        diffs, first = np.zeros(n, dtype=DIFF_DTYPE), ctypes.c_int(-1)
        self._check(self._lib.qoimi_compare_images(self._h, d_a, m.a_offsets, a_channels, d_b, m.b_offsets, b_channels, m.descs, n,
                                                   _ptr(diffs, ImageDiff), ctypes.byref(first), stream), "qoimi_compare_images")
        return diffs, first.value

    # ---- decode and what reads a pack ------------------------------------------------------------------------------------------
    def decode_batch(self, d_streams: int, stream_stride: int, sizes: Sequence[int], descs: Sequence[QoiDesc],
                     channels: int, d_pixels: int, pixel_stride: int, stream: int = 0) -> None:
        n = len(sizes)
        if len(descs) != n:
            raise QoiError(f"decode_batch: {n} sizes but {len(descs)} descriptors")
        if isinstance(sizes, ctypes.Array) and isinstance(descs, ctypes.Array):
            c_sizes, c_descs = sizes, descs               # the caller's own C arrays (int[n], qoi_desc[n]): handed through as they are
        else:
            if n > 1 and any(int(sz) > stream_stride for sz in sizes):
                raise QoiError("decode_batch: a stream is longer than stream_stride")
            m = self._pointers(dict(sizes=sizes, descs=descs), wraps=True)
            c_sizes, c_descs = m.sizes, m.descs
        self._check(self._lib.qoimi_decode_batch(self._h, d_streams, stream_stride, c_sizes, c_descs, n, channels,
                                                 d_pixels, pixel_stride, stream), "qoimi_decode_batch")

    def decode_images(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc],
                      channels: int, d_pixels: int, pixel_offsets: Sequence[int], stream: int = 0) -> None:
        """Streams and images at per-image byte offsets, any order (``qoimi_decode_images``): image i is written tightly packed."""
        n = len(sizes)
        m = self._marshal("decode_images", "stream offset, size, descriptor and pixel offset per image", n, wraps=True,
                          stream_offsets=stream_offsets, pixel_offsets=pixel_offsets, sizes=sizes, descs=descs)
        self._check(self._lib.qoimi_decode_images(self._h, d_streams, m.stream_offsets, m.sizes, m.descs, n, channels, d_pixels, m.pixel_offsets, stream),
                    "qoimi_decode_images")

    def read_descs(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], stream: int = 0):
        """The headers of the streams of a pack: (descs, first_bad) - first_bad is None when every stream passes the rules of
        qoi.h:497-521, else the lowest failing index (``qoimi_read_descs`` then returns QOIMI_E_ARG; the descriptors are filled anyway)."""
        n = len(sizes)
        m = self._marshal("read_descs", "stream offset per size", n, wraps=True, stream_offsets=stream_offsets, sizes=sizes)
        descs = (QoiDesc * n)()
        bad = ctypes.c_int(-1)
        rc = self._lib.qoimi_read_descs(self._h, d_streams, m.stream_offsets, m.sizes, n, descs, ctypes.byref(bad), stream)
        if rc != 0 and bad.value < 0:
            self._check(rc, "qoimi_read_descs")
        return list(descs), (bad.value if bad.value >= 0 else None)

    def inspect_streams(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], stream: int = 0):
        """Chunk statistics and strict checks of the streams of a pack (``qoimi_inspect_streams``): (infos, first_flagged) - infos is a
        numpy array of ``streaminfo.INFO_DTYPE``, first_flagged the lowest index with flags != 0 or None."""
        from .streaminfo import INFO_DTYPE
        n = len(sizes)
        m = self._marshal("inspect_streams", "stream offset per size", n, stream_offsets=stream_offsets, sizes=sizes)
        infos, first = np.zeros(n, dtype=INFO_DTYPE), ctypes.c_int(-1)
        self._check(self._lib.qoimi_inspect_streams(self._h, d_streams, m.stream_offsets, m.sizes, n, _ptr(infos, StreamInfo), ctypes.byref(first), stream),
                    "qoimi_inspect_streams")
        return infos, (first.value if first.value >= 0 else None)

    def decode_thumbnails(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                          factors, mode: int, d_thumbs: int, thumb_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """Every image of a pack at 1/f of its size (``qoimi_decode_thumbnails``, synchronous, through bounded staging): thumbnail i is
        written tightly packed at d_thumbs + thumb_offsets[i].  factors: one int for all images or one per image, each 1..64;
        mode: ``thumbs.PLAIN`` or ``thumbs.ALPHA_WEIGHTED``; ``qoi_amd/thumbs.py: thumbnail`` states the result."""
        n = len(sizes)
        seqs = self._per_image("decode_thumbnails", "stream offset, size, descriptor, factor and thumbnail offset per image", n,
                               stream_offsets=stream_offsets, sizes=sizes, descs=descs, thumb_offsets=thumb_offsets, factors=factors)
        if any(not 0 <= int(f) < 2 ** 32 for f in seqs["factors"]):
            raise QoiError("decode_thumbnails: a factor outside 1..64")
        m = self._pointers(seqs)
        self._check(self._lib.qoimi_decode_thumbnails(self._h, d_streams, m.stream_offsets, m.sizes, m.descs, n, channels, m.factors, mode,
                                                      d_thumbs, m.thumb_offsets, staging_bytes, stream), "qoimi_decode_thumbnails")

    def _gather(self, what: str, cls, d_streams, stream_offsets, sizes, descs, channels, items, more, d_out, out_offsets, staging_bytes, stream,
                index=None, each=None, f=None) -> None:
        """The gather call ``qoimi_<what>`` over items of the structure cls - `more` stands between the items and the outputs, then the
        format f, where given - or, with index = (interval_rows, points, point_firsts), its indexed form: the same call, those appended."""
        m = self._gather_args(what, cls, items, stream_offsets, sizes, descs, out_offsets, index, each=each)
        if f is not None:
            more += (ctypes.byref(tensor_format(f)),)
        self._check(getattr(self._lib, "qoimi_" + what)(self._h, d_streams, m.stream_offsets, m.sizes, m.descs, m.n, channels, m.items, len(m.items), *more,
                                                        d_out, m.out_offsets, staging_bytes, stream, *m.index), "qoimi_" + what)

    def decode_crops(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                     crops, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """Rectangles of a pack's images (``qoimi_decode_crops``, synchronous, through bounded staging): output j is written tightly packed at
        d_out + out_offsets[j].  crops: ``QoimiCrop`` structures or (image, x, y, width, height, flags) tuples, flags of ``crops.FLIP_X`` /
        ``crops.FLIP_Y``; an image no crop names is not decoded; ``qoi_amd/crops.py: crop`` states the result."""
        self._gather("decode_crops", QoimiCrop, d_streams, stream_offsets, sizes, descs, channels, crops, (), d_out, out_offsets, staging_bytes, stream)

    def decode_crops_indexed(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                             crops, d_out: int, out_offsets: Sequence[int], interval_rows, points, point_firsts: Sequence[int],
                             staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_crops`` byte for byte, decoding every referenced image only from the last seek row at or above its topmost crop
        (``qoimi_decode_crops_indexed``).  interval_rows, points, point_firsts: as ``build_seek_index`` took and returned them;
        ``crop_stats`` then holds the counters of the inner call over the band streams."""
        self._gather("decode_crops_indexed", QoimiCrop, d_streams, stream_offsets, sizes, descs, channels, crops, (), d_out, out_offsets, staging_bytes, stream,
                     (interval_rows, points, point_firsts), each="stream offset, size, descriptor, interval and first point per image")

    def decode_resized(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                       items, mode: int, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """Rectangles of a pack's images resampled to fixed sizes (``qoimi_decode_resized``, synchronous, through bounded staging): output j
        is written tightly packed at d_out + out_offsets[j].  items: ``QoimiResize`` structures or (image, x, y, width, height, out_width,
        out_height, flags) tuples, flags of ``resize.FLIP_X`` / ``resize.FLIP_Y``; mode: ``resize.PLAIN`` or ``resize.ALPHA_WEIGHTED``; an image
        no item names is not decoded; ``qoi_amd/resize.py: resize`` states the result."""
        self._gather("decode_resized", QoimiResize, d_streams, stream_offsets, sizes, descs, channels, items, (mode,), d_out, out_offsets, staging_bytes, stream)

    def decode_resized_indexed(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                               items, mode: int, d_out: int, out_offsets: Sequence[int], interval_rows, points, point_firsts: Sequence[int],
                               staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_resized`` byte for byte, decoding every referenced image only from the last seek row at or above its topmost source
        rectangle (``qoimi_decode_resized_indexed``).  interval_rows, points, point_firsts: as ``build_seek_index`` took and returned them;
        ``resize_stats`` then holds the counters of the inner call over the band streams."""
        self._gather("decode_resized_indexed", QoimiResize, d_streams, stream_offsets, sizes, descs, channels, items, (mode,), d_out, out_offsets, staging_bytes,
                     stream, (interval_rows, points, point_firsts))

    def decode_bilinear(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                        items, mode: int, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_resized`` with the antialiased bilinear (triangle) filter (``qoimi_decode_bilinear``, synchronous, through bounded
        staging): the same items, modes, flips and outputs; a rectangle is reduced by at most 32 per axis and
        max(width, out_width) * max(height, out_height) stays below 2**30; ``qoi_amd/bilinear.py: bilinear`` states the result."""
        self._gather("decode_bilinear", QoimiResize, d_streams, stream_offsets, sizes, descs, channels, items, (mode,), d_out, out_offsets, staging_bytes, stream)

    def decode_bilinear_indexed(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                                items, mode: int, d_out: int, out_offsets: Sequence[int], interval_rows, points, point_firsts: Sequence[int],
                                staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_bilinear`` byte for byte, decoding every referenced image only from the last seek row at or above its topmost source
        rectangle (``qoimi_decode_bilinear_indexed``).  interval_rows, points, point_firsts: as ``build_seek_index`` took and returned them;
        ``bilinear_stats`` then holds the counters of the inner call over the band streams."""
        self._gather("decode_bilinear_indexed", QoimiResize, d_streams, stream_offsets, sizes, descs, channels, items, (mode,), d_out, out_offsets, staging_bytes,
                     stream, (interval_rows, points, point_firsts))

    def decode_warped(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                      items, mode: int, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """Rectangles of a pack's images sampled through an affine map with bilinear weights (``qoimi_decode_warped``, synchronous, through
        bounded staging): output j is written tightly packed at d_out + out_offsets[j].  items: ``QoimiWarp`` structures or the tuples of
        ``warp.fields`` (``warp.item`` makes one; the flag ``warp.NEAREST`` takes one sample instead of 2 x 2 taps - for label maps -, ``warp.BICUBIC`` = 16 takes 4 x 4 under Keys' cubic; ``warp.REFLECT`` = 64, ``warp.REFLECT_101`` = 128 and ``warp.WRAP`` = 256 fold every tap into the rectangle instead of ``warp.REPLICATE`` or the fill; ``warp.SUPER2`` = 1024 and ``warp.SUPER4`` = 2048 average 2 x 2 or 4 x 4 bilinear sub-samples per output pixel with one rounding, for maps that reduce by up to 4; ``warp.VOTE2`` = 8192 and ``warp.VOTE4`` = 16384 take the majority vote of 2 x 2 or 4 x 4 nearest sub-samples per output pixel - for label maps under such maps -, a sampling of their own; ``warp.PROJECTIVE`` = 131072 makes the map a perspective map whose two coefficients g and h travel in ``reserved`` - ``warp.item(..., proj=(g, h))``, ``warp.perspective`` -, with the bilinear, nearest or bicubic sampling and any border); mode: ``warp.PLAIN`` or ``warp.ALPHA_WEIGHTED``; an image no item names is not decoded;
        ``qoi_amd/warp.py: warp`` states the result."""
        self._gather("decode_warped", QoimiWarp, d_streams, stream_offsets, sizes, descs, channels, items, (mode,), d_out, out_offsets, staging_bytes, stream)

    def decode_warped_indexed(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                              items, mode: int, d_out: int, out_offsets: Sequence[int], interval_rows, points, point_firsts: Sequence[int],
                              staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_warped`` byte for byte, decoding every referenced image only from the last seek row at or above its topmost source
        rectangle (``qoimi_decode_warped_indexed``).  interval_rows, points, point_firsts: as ``build_seek_index`` took and returned them;
        ``warp_stats`` then holds the counters of the inner call over the band streams."""
        self._gather("decode_warped_indexed", QoimiWarp, d_streams, stream_offsets, sizes, descs, channels, items, (mode,), d_out, out_offsets, staging_bytes,
                     stream, (interval_rows, points, point_firsts))

    def decode_tensors(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                       items, filter: int, mode: int, f, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_resized`` (filter ``tensors.FILTER_AREA``), ``decode_bilinear`` (``tensors.FILTER_BILINEAR``) or the antialiased bicubic
        filter ``qoi_amd/bicubic.py`` states (``tensors.FILTER_BICUBIC``; it has no u8 call: U8 with HWC gives its bytes) or the Lanczos filter of
        ``qoi_amd/lanczos.py`` (``tensors.FILTER_LANCZOS``, likewise) or the nearest filter of ``qoi_amd/nearest.py`` for label maps
        (``tensors.FILTER_NEAREST``, likewise) or the majority vote of ``qoi_amd/mode.py`` for reducing them (``tensors.FILTER_MODE`` = 11,
        likewise) with the outputs written
        as tensors (``qoimi_decode_tensors``, synchronous, through bounded staging): f is a ``QoimiTensorFormat`` or the tuple of
        ``tensors.fmt`` - u8, f16, bf16 or f32 elements, HWC or CHW, each channel scaled and shifted, or i32 / i64 class indices, and HW: the
        first channel as one plane, or HW_ID24 (i32 / i64 only): ``r | g << 8 | b << 16`` as one plane of 24-bit ids; every d_out + out_offsets[j] is a
        multiple of the element size; ``qoi_amd/tensors.py: tensors`` states the result."""
        self._gather("decode_tensors", QoimiResize, d_streams, stream_offsets, sizes, descs, channels, items, (filter, mode), d_out, out_offsets, staging_bytes,
                     stream, f=f)

    def decode_warped_tensors(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], channels: int,
                              items, mode: int, f, d_out: int, out_offsets: Sequence[int], staging_bytes: int = 0, stream: int = 0) -> None:
        """``decode_warped`` with the outputs written as tensors (``qoimi_decode_warped_tensors``): f and the outputs as for
        ``decode_tensors``; ``qoi_amd/tensors.py: warped_tensors`` states the result."""
        self._gather("decode_warped_tensors", QoimiWarp, d_streams, stream_offsets, sizes, descs, channels, items, (mode,), d_out, out_offsets, staging_bytes,
                     stream, f=f)

    def _pixel_stats(self, what: str, d_streams, stream_offsets, sizes, descs, regions, d_hist, staging_bytes, stream, index=None) -> List[QoimiPixelStat]:
        m = self._gather_args(what, QoimiCrop, regions, stream_offsets, sizes, descs, index=index, noun="region")
        out = (QoimiPixelStat * max(len(m.items), 1))()
        self._check(getattr(self._lib, "qoimi_" + what)(self._h, d_streams, m.stream_offsets, m.sizes, m.descs, m.n, m.items, len(m.items), out, d_hist or None,
                                                        staging_bytes, stream, *m.index), "qoimi_" + what)
        return list(out)[:len(m.items)]

    def pixel_stats(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], regions,
                    d_hist: int = 0, staging_bytes: int = 0, stream: int = 0) -> List[QoimiPixelStat]:
        """Pixel statistics of rectangles of a pack's images (``qoimi_pixel_stats``, synchronous, through bounded staging): one
        ``QoimiPixelStat`` per region.  regions: ``QoimiCrop`` structures or (image, x, y, width, height, flags) tuples; d_hist: 0, or device
        memory of 4096 bytes per region that receives uint32[n_regions][4][256]; an image no region names is not decoded;
        ``qoi_amd/pixelstats.py: stats`` states the result."""
        return self._pixel_stats("pixel_stats", d_streams, stream_offsets, sizes, descs, regions, d_hist, staging_bytes, stream)

    def pixel_stats_indexed(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], regions,
                            interval_rows, points, point_firsts: Sequence[int], d_hist: int = 0, staging_bytes: int = 0,
                            stream: int = 0) -> List[QoimiPixelStat]:
        """``pixel_stats`` field for field, decoding every referenced image only from the last seek row at or above its topmost region
        (``qoimi_pixel_stats_indexed``).  interval_rows, points, point_firsts: as ``build_seek_index`` took and returned them;
        ``pixel_stats_counters`` then holds the counters of the inner call over the band streams."""
        return self._pixel_stats("pixel_stats_indexed", d_streams, stream_offsets, sizes, descs, regions, d_hist, staging_bytes, stream,
                                 (interval_rows, points, point_firsts))

    # ---- the seek index ---------------------------------------------------------------------------------------------------------
    def build_seek_index(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc],
                         interval_rows, staging_bytes: int = 0, stream: int = 0):
        """The seek points of every image of a pack (``qoimi_build_seek_index``, synchronous: one inspect plus one full decode): (points,
        point_firsts) - points a numpy array of ``seekindex.POINT_DTYPE``, the images' points back to back, image i's from point_firsts[i]
        on.  interval_rows: one int for all images or one per image, each with interval_rows * width >= 128; ``qoi_amd/seekindex.py:
        points`` states the result."""
        n = len(sizes)
        seqs = self._per_image("build_seek_index", "stream offset, size, descriptor and interval per image", n,
                               stream_offsets=stream_offsets, sizes=sizes, descs=descs, interval_rows=interval_rows)
        points, firsts, room = self._seek_index_room("build_seek_index", descs, seqs["interval_rows"])
        m = self._pointers(seqs)
        self._check(self._lib.qoimi_build_seek_index(self._h, d_streams, m.stream_offsets, m.sizes, m.descs, n, m.interval_rows, room, staging_bytes, stream),
                    "qoimi_build_seek_index")
        return points, firsts

    def seek_index_from_pixels(self, d_pixels: int, pixel_offsets: Sequence[int], d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int],
                               descs: Sequence[QoiDesc], interval_rows, stream: int = 0):
        """``build_seek_index`` for whoever holds the pixels the pack was encoded from (``qoimi_seek_index_from_pixels``, synchronous: one
        inspect and two kernels over the pixels, no decode, no staging): image i is width * height * channels bytes at d_pixels +
        pixel_offsets[i], any byte offset.  Returns (points, point_firsts) as ``build_seek_index`` does; that stream i decodes to those
        pixels is not checked (``verify_images`` does that); ``qoi_amd/seekindex.py: points_from_pixels`` states the result."""
        n = len(sizes)
        seqs = self._per_image("seek_index_from_pixels", "pixel offset, stream offset, size, descriptor and interval per image", n,
                               pixel_offsets=pixel_offsets, stream_offsets=stream_offsets, sizes=sizes, descs=descs, interval_rows=interval_rows)
        points, firsts, room = self._seek_index_room("seek_index_from_pixels", descs, seqs["interval_rows"])
        m = self._pointers(seqs)
        self._check(self._lib.qoimi_seek_index_from_pixels(self._h, d_pixels, m.pixel_offsets, d_streams, m.stream_offsets, m.sizes, m.descs, n,
                                                           m.interval_rows, room, stream), "qoimi_seek_index_from_pixels")
        return points, firsts

    def make_band_streams(self, d_streams: int, stream_offsets: Sequence[int], sizes: Sequence[int], descs: Sequence[QoiDesc], interval_rows,
                          points, point_firsts: Sequence[int], bands, d_out: int, out_offsets: Sequence[int], stream: int = 0) -> List[QoimiBandInfo]:
        """Band streams written on the device (``qoimi_make_band_streams``, synchronous): band stream j at d_out + out_offsets[j]; returns
        one ``QoimiBandInfo`` per band.  bands: ``QoimiBand`` structures or (image, first_row, rows) tuples; points, point_firsts: as
        ``build_seek_index`` returns them; ``qoi_amd/seekindex.py: band_stream`` states the result."""
        m = self._gather_args("make_band_streams", QoimiBand, bands, stream_offsets, sizes, descs, out_offsets, (interval_rows, points, point_firsts),
                              each="stream offset, size, descriptor, interval and first point per image")
        infos = (QoimiBandInfo * max(len(m.items), 1))()
        self._check(self._lib.qoimi_make_band_streams(self._h, d_streams, m.stream_offsets, m.sizes, m.descs, m.n, *m.index, m.items, len(m.items), d_out,
                                                      m.out_offsets, infos, stream), "qoimi_make_band_streams")
        return list(infos)[:len(m.items)]

    # ---- counters of the last call of a kind ------------------------------------------------------------------------------------
    def tile_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``encode_tiles`` call: (sub-batches, launches of the gather kernel, bytes of staging planned, images referenced)."""
        return self._four_counters("tile_stats")

    def thumbnail_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_thumbnails`` call: (sub-batches decoded, launches of the reduction kernel, bytes of staging planned, 0)."""
        return self._four_counters("thumbnail_stats")

    def crop_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_crops`` call: (sub-batches decoded, launches of the gather kernel, bytes of staging planned, images decoded)."""
        return self._four_counters("crop_stats")

    def resize_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_resized`` call: (sub-batches decoded, launches of the filter kernel, bytes of staging planned, images decoded)."""
        return self._four_counters("resize_stats")

    def bilinear_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_bilinear`` call: (sub-batches decoded, launches of the filter kernel, bytes of staging planned, images decoded)."""
        return self._four_counters("bilinear_stats")

    def warp_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_warped`` call: (sub-batches decoded, launches of the warp kernel, bytes of staging planned, images decoded)."""
        return self._four_counters("warp_stats")

    def tensor_stats(self) -> Tuple[int, int, int, int]:
        """Of the last ``decode_tensors`` or ``decode_warped_tensors`` call: (sub-batches decoded, launches of the tensor kernel, bytes of
        staging planned, images decoded)."""
        return self._four_counters("tensor_stats")

    def pixel_stats_counters(self) -> Tuple[int, int, int, int]:
        """Of the last ``pixel_stats`` call: (sub-batches decoded, launches of the reduction kernel, bytes of staging planned, images decoded)."""
        return self._four_counters("pixel_stats_counters")

    def seek_stats(self) -> Tuple[int, int, int, int]:
        """(sub-batches decoded by the last ``build_seek_index``; of the last ``make_band_streams`` / indexed call: band streams
        assembled, bytes of the band arena planned, stream bytes copied)."""
        return self._four_counters("seek_stats")

    def decode_stats(self) -> dict:
        rounds, redo, segments, fallback = self._four_counters("decode_stats")
        return {"rounds": rounds, "redo_segments": redo, "segments": segments, "sync_fallback_segments": fallback}

    # ---- the rest ---------------------------------------------------------------------------------------------------------------
    def synth_frames(self, kind: int, seed: int, first_frame: int, n_frames: int, width: int, height: int,
                     d_pixels: int, pixel_stride: int, stream: int = 0) -> None:
        self._check(self._lib.qoimi_synth_frames(self._h, kind, seed, first_frame, n_frames, width, height,
                                                 d_pixels, pixel_stride, stream), "qoimi_synth_frames")

    def hash_streams(self, d_streams: int, stream_stride: int, d_stream_len: int, n_streams: int, d_hash: int, stream: int = 0) -> None:
        """64-bit content hash of every stream into the device array d_hash (uint64[n_streams]); synth.stream_hash64 is the same function."""
        self._check(self._lib.qoimi_hash_streams(self._h, d_streams, stream_stride, d_stream_len, n_streams, d_hash, stream), "qoimi_hash_streams")

    def set_profiling(self, on: bool) -> None:
        self._check(self._lib.qoimi_set_profiling(self._h, 1 if on else 0), "qoimi_set_profiling")

    def get_profile(self, stream: int = 0) -> dict:
        """kernel name -> (accumulated ms, launches) since profiling was enabled (syncs stream)."""
        ms = (ctypes.c_double * 64)()
        calls = (ctypes.c_longlong * 64)()
        n = min(64, self._lib.qoimi_get_profile(self._h, stream, ms, calls, 64))
        return {self._lib.qoimi_kernel_name(i).decode(): (ms[i], calls[i]) for i in range(1, n)}

    def workspace_bytes(self) -> dict:
        """Device bytes the context's arenas hold: encode workspace (with the staging of ``encode_packed`` and ``encode_tiles``), decode workspace (with the tables of ``inspect_streams`` and ``compare_images`` and the staging of ``verify_images`` / ``decode_thumbnails`` / ``decode_crops`` / ``decode_resized`` / ``decode_bilinear`` / ``pixel_stats``, the tables of ``build_seek_index`` / ``seek_index_from_pixels`` and the band arena of the indexed calls), staging of the host-pointer entry points."""
        out = (ctypes.c_size_t * 3)()
        self._lib.qoimi_workspace_bytes(self._h, out)
        return {"encode": int(out[0]), "decode": int(out[1]), "staging": int(out[2])}

    def set_decode_record_cap(self, nbytes: int, release: bool = False) -> None:
        """Caps the chunk-record arena of decode calls (larger calls run as sub-batches of whole images); release=True frees the arena grown so far."""
        self._check(self._lib.qoimi_set_decode_record_cap(self._h, int(nbytes), 1 if release else 0), "qoimi_set_decode_record_cap")
