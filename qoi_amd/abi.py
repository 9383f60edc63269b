"""The C ABI of libqoi_mi355x.so as ctypes sees it: the structures of include/qoi_mi355x.h and one prototype table for its functions.

``api.load_library`` applies ``PROTOTYPES``; tests/test_abi.py checks the table and the structures against the header, type by type.
"""
import ctypes


class QoiDesc(ctypes.Structure):
    """``qoi_desc`` (qoi.h:236-241)."""
    _fields_ = [("width", ctypes.c_uint), ("height", ctypes.c_uint),
                ("channels", ctypes.c_ubyte), ("colorspace", ctypes.c_ubyte)]

    def __repr__(self):
        return f"QoiDesc({self.width}x{self.height}, channels={self.channels}, colorspace={self.colorspace})"


class StreamInfo(ctypes.Structure):
    """``qoimi_stream_info``: 64 bytes, the layout of ``streaminfo.INFO_DTYPE``."""
    _fields_ = [("pixels", ctypes.c_ulonglong), ("run_pixels", ctypes.c_ulonglong), ("ops", ctypes.c_uint * 6),
                ("repeat_index", ctypes.c_uint), ("walk_end", ctypes.c_uint), ("flags", ctypes.c_uint), ("reserved", ctypes.c_uint * 3)]


class ImageDiff(ctypes.Structure):
    """``qoimi_image_diff``: 32 bytes, the layout of ``imagediff.DIFF_DTYPE``."""
    _fields_ = [("mismatched", ctypes.c_ulonglong), ("first", ctypes.c_ulonglong), ("want", ctypes.c_uint), ("got", ctypes.c_uint),
                ("flags", ctypes.c_uint), ("reserved", ctypes.c_uint)]


class QoimiCrop(ctypes.Structure):
    """``qoimi_crop``: 24 bytes - a rectangle of image ``image`` and how it is mirrored (``crops.FLIP_X`` / ``crops.FLIP_Y``)."""
    _fields_ = [("image", ctypes.c_uint), ("x", ctypes.c_uint), ("y", ctypes.c_uint), ("width", ctypes.c_uint), ("height", ctypes.c_uint),
                ("flags", ctypes.c_uint)]


assert ctypes.sizeof(QoimiCrop) == 24 and [getattr(QoimiCrop, f).offset for f, _ in QoimiCrop._fields_] == [0, 4, 8, 12, 16, 20]


class QoimiTile(ctypes.Structure):
    """``qoimi_tile``: 32 bytes - a rectangle of image ``image``, the factor it is box-reduced by and how the result is mirrored
    (``tiles.FLIP_X`` / ``tiles.FLIP_Y``); ``reserved`` is 0."""
    _fields_ = [("image", ctypes.c_uint), ("x", ctypes.c_uint), ("y", ctypes.c_uint), ("width", ctypes.c_uint), ("height", ctypes.c_uint),
                ("factor", ctypes.c_uint), ("flags", ctypes.c_uint), ("reserved", ctypes.c_uint)]


assert ctypes.sizeof(QoimiTile) == 32 and [getattr(QoimiTile, f).offset for f, _ in QoimiTile._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]


class QoimiResize(ctypes.Structure):
    """``qoimi_resize``: 32 bytes - a rectangle of image ``image``, the size it is resampled to and how the result is mirrored
    (``resize.FLIP_X`` / ``resize.FLIP_Y``)."""
    _fields_ = [("image", ctypes.c_uint), ("x", ctypes.c_uint), ("y", ctypes.c_uint), ("width", ctypes.c_uint), ("height", ctypes.c_uint),
                ("out_width", ctypes.c_uint), ("out_height", ctypes.c_uint), ("flags", ctypes.c_uint)]


assert ctypes.sizeof(QoimiResize) == 32 and [getattr(QoimiResize, f).offset for f, _ in QoimiResize._fields_] == [0, 4, 8, 12, 16, 20, 24, 28]


class QoimiWarp(ctypes.Structure):
    """``qoimi_warp``: 72 bytes - a rectangle of image ``image``, the size of the output, the inverse affine map from the output into the
    rectangle (``warp.py`` states it), the border (``warp.REPLICATE`` or ``fill``); ``reserved`` is 0, or with ``warp.PROJECTIVE`` the two
    perspective coefficients as 16-bit halves (``warp.proj_reserved``)."""
    _fields_ = [("image", ctypes.c_uint), ("x", ctypes.c_uint), ("y", ctypes.c_uint), ("width", ctypes.c_uint), ("height", ctypes.c_uint),
                ("out_width", ctypes.c_uint), ("out_height", ctypes.c_uint), ("flags", ctypes.c_uint), ("a", ctypes.c_int), ("b", ctypes.c_int),
                ("d", ctypes.c_int), ("e", ctypes.c_int), ("fill", ctypes.c_uint), ("reserved", ctypes.c_uint), ("c", ctypes.c_longlong),
                ("f", ctypes.c_longlong)]


assert ctypes.sizeof(QoimiWarp) == 72 and [getattr(QoimiWarp, f).offset for f, _ in QoimiWarp._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 64]


class QoimiTensorFormat(ctypes.Structure):
    """``qoimi_tensor_format``: 48 bytes - the element type (``tensors.U8`` / ``F16`` / ``BF16`` / ``F32``), the layout (``tensors.HWC`` /
    ``CHW``) and the scale and bias of each channel (``tensors.py`` states the result)."""
    _fields_ = [("dtype", ctypes.c_uint), ("layout", ctypes.c_uint), ("scale", ctypes.c_float * 4), ("bias", ctypes.c_float * 4),
                ("reserved", ctypes.c_uint * 2)]


assert ctypes.sizeof(QoimiTensorFormat) == 48 and [getattr(QoimiTensorFormat, f).offset for f, _ in QoimiTensorFormat._fields_] == [0, 4, 8, 24, 40]


class QoimiPixelStat(ctypes.Structure):
    """``qoimi_pixel_stat``: 128 bytes - what ``qoimi_pixel_stats`` says of one region (``pixelstats.stats`` states the fields)."""
    _fields_ = [("pixels", ctypes.c_ulonglong), ("sum", ctypes.c_ulonglong * 4), ("sum_sq", ctypes.c_ulonglong * 4), ("min", ctypes.c_ubyte * 4),
                ("max", ctypes.c_ubyte * 4), ("first", ctypes.c_uint), ("flags", ctypes.c_uint), ("opaque_pixels", ctypes.c_ulonglong),
                ("transparent_pixels", ctypes.c_ulonglong), ("grey_pixels", ctypes.c_ulonglong), ("reserved", ctypes.c_uint * 4)]


assert ctypes.sizeof(QoimiPixelStat) == 128 and [getattr(QoimiPixelStat, f).offset for f, _ in QoimiPixelStat._fields_] == [0, 8, 40, 72, 76, 80, 84, 88, 96, 104, 112]


class QoimiSeekPoint(ctypes.Structure):
    """``qoimi_seek_point``: 272 bytes, the layout of ``seekindex.POINT_DTYPE`` - the decoder's state at a row boundary."""
    _fields_ = [("byte_off", ctypes.c_uint), ("skip", ctypes.c_uint), ("prev", ctypes.c_uint), ("reserved", ctypes.c_uint), ("table", ctypes.c_uint * 64)]


class QoimiBand(ctypes.Structure):
    """``qoimi_band``: 16 bytes - rows [first_row, first_row + rows) of image ``image``; first_row is 0 or a seek row."""
    _fields_ = [("image", ctypes.c_uint), ("first_row", ctypes.c_uint), ("rows", ctypes.c_uint), ("reserved", ctypes.c_uint)]


class QoimiBandInfo(ctypes.Structure):
    """``qoimi_band_info``: 24 bytes - what a band stream will be: its size, its descriptor and the rows in front of the band's own."""
    _fields_ = [("size", ctypes.c_ulonglong), ("desc", QoiDesc), ("pad_rows", ctypes.c_uint)]


assert ctypes.sizeof(QoimiSeekPoint) == 272 and [getattr(QoimiSeekPoint, f).offset for f, _ in QoimiSeekPoint._fields_] == [0, 4, 8, 12, 16]
assert ctypes.sizeof(QoimiBand) == 16 and ctypes.sizeof(QoimiBandInfo) == 24 and (QoimiBandInfo.desc.offset, QoimiBandInfo.pad_rows.offset) == (8, 20)


def _prototypes():
    P = ctypes.POINTER
    vp, sz, ci, cu, ll, cs = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint, ctypes.c_longlong, ctypes.c_char_p
    szp, cip, cup, llp, ullp = P(sz), P(ci), P(cu), P(ll), P(ctypes.c_ulonglong)
    desc, crop, tile, resize, warp, fmt = P(QoiDesc), P(QoimiCrop), P(QoimiTile), P(QoimiResize), P(QoimiWarp), P(QoimiTensorFormat)
    point, band, info = P(QoimiSeekPoint), P(QoimiBand), P(QoimiBandInfo)
    # vp where the header says void* (device addresses and streams arrive as ints) and for the qoimi_ctx*
    pack = [vp, vp, szp, cip, desc, ci]            # ctx, d_streams, stream_offsets, sizes, descs, n_images: how a call over a pack begins
    out = [vp, szp, sz, vp]                        # d_out, out_offsets, staging_bytes, stream: how a gather call ends
    index = [cup, point, szp]                      # interval_rows, points, point_firsts: what an indexed call adds
    packed = [cu, vp, sz, vp, vp, sz, ullp, cip]   # align, d_packed, capacity, d_packed_off, d_stream_len, staging, the two host tables
    stats = (None, [vp, llp])
    return {
        "qoi_encode": (vp, [vp, desc, cip]),
        "qoi_decode": (vp, [vp, ci, desc, ci]),
        "qoi_write": (ci, [cs, vp, desc]),
        "qoi_read": (vp, [cs, desc, ci]),
        "qoimi_ctx_create": (ci, [ci, P(vp)]),
        "qoimi_ctx_destroy": (None, [vp]),
        "qoimi_last_error": (cs, []),
        "qoimi_encode_bound": (sz, [desc]),
        "qoimi_encode_batch": (ci, [vp, vp, sz, desc, ci, vp, sz, vp, vp]),
        "qoimi_encode_images": (ci, [vp, vp, szp, desc, ci, vp, szp, vp, vp]),
        "qoimi_encode_suspect_calls": (ll, [vp]),
        "qoimi_encode_status": (ci, [vp, vp]),
        "qoimi_set_encode_small_call_order": (ci, [vp, ci]),
        "qoimi_encode_retries": (ll, [vp]),
        "qoimi_decode_batch": (ci, [vp, vp, sz, cip, desc, ci, ci, vp, sz, vp]),
        "qoimi_decode_images": (ci, pack + [ci, vp, szp, vp]),
        "qoimi_pack_streams": (ci, [vp, vp, sz, vp, ci, cu, vp, sz, vp, vp]),
        "qoimi_encode_packed": (ci, [vp, vp, sz, desc, ci] + packed + [vp]),
        "qoimi_encode_images_packed": (ci, [vp, vp, szp, desc, ci] + packed + [vp]),
        "qoimi_encode_tiles": (ci, [vp, vp, szp, desc, ci, ci, tile, ci, ci] + packed + [desc, vp]),
        "qoimi_tile_size": (sz, [desc, tile, ci, cup, cup]),
        "qoimi_tile_pyramid": (ci, [desc, cu, cu, cu, tile, ci]),
        "qoimi_tile_stats": stats,
        "qoimi_read_descs": (ci, [vp, vp, szp, cip, ci, desc, cip, vp]),
        "qoimi_inspect_streams": (ci, [vp, vp, szp, cip, ci, P(StreamInfo), cip, vp]),
        "qoimi_compare_images": (ci, [vp, vp, szp, ci, vp, szp, ci, desc, ci, P(ImageDiff), cip, vp]),
        "qoimi_verify_images": (ci, [vp, vp, szp, desc, ci, vp, szp, cip, sz, P(ImageDiff), cip, vp]),
        "qoimi_decode_thumbnails": (ci, pack + [ci, cup, ci] + out),
        "qoimi_thumbnail_size": (sz, [desc, cu, ci, cup, cup]),
        "qoimi_thumbnail_stats": stats,
        "qoimi_decode_crops": (ci, pack + [ci, crop, ci] + out),
        "qoimi_crop_size": (sz, [desc, crop, ci]),
        "qoimi_crop_stats": stats,
        "qoimi_decode_resized": (ci, pack + [ci, resize, ci, ci] + out),
        "qoimi_resize_size": (sz, [desc, resize, ci]),
        "qoimi_resize_stats": stats,
        "qoimi_decode_bilinear": (ci, pack + [ci, resize, ci, ci] + out),
        "qoimi_bilinear_size": (sz, [desc, resize, ci]),
        "qoimi_bilinear_stats": stats,
        "qoimi_decode_warped": (ci, pack + [ci, warp, ci, ci] + out),
        "qoimi_warp_size": (sz, [desc, warp, ci]),
        "qoimi_warp_stats": stats,
        "qoimi_warp_orient": (ci, [desc, cu, cu, cu, cu, ci, warp]),
        "qoimi_decode_tensors": (ci, pack + [ci, resize, ci, ci, ci, fmt] + out),
        "qoimi_decode_warped_tensors": (ci, pack + [ci, warp, ci, ci, fmt] + out),
        "qoimi_tensor_size": (sz, [desc, resize, ci, ci, fmt]),
        "qoimi_warp_tensor_size": (sz, [desc, warp, ci, fmt]),
        "qoimi_tensor_stats": stats,
        "qoimi_pixel_stats": (ci, pack + [crop, ci, P(QoimiPixelStat), vp, sz, vp]),
        "qoimi_pixel_stats_counters": stats,
        "qoimi_seek_points": (ci, [desc, cu]),
        "qoimi_build_seek_index": (ci, pack + [cup, point, sz, vp]),
        "qoimi_seek_index_from_pixels": (ci, [vp, vp, szp, vp, szp, cip, desc, ci, cup, point, vp]),
        "qoimi_band_plan": (ci, [desc, ci, cu, point, band, info]),
        "qoimi_make_band_streams": (ci, pack + index + [band, ci, vp, szp, info, vp]),
        "qoimi_decode_crops_indexed": (ci, pack + [ci, crop, ci] + out + index),
        "qoimi_decode_resized_indexed": (ci, pack + [ci, resize, ci, ci] + out + index),
        "qoimi_decode_bilinear_indexed": (ci, pack + [ci, resize, ci, ci] + out + index),
        "qoimi_decode_warped_indexed": (ci, pack + [ci, warp, ci, ci] + out + index),
        "qoimi_pixel_stats_indexed": (ci, pack + [crop, ci, P(QoimiPixelStat), vp, sz, vp] + index),
        "qoimi_seek_stats": stats,
        "qoimi_synth_frames": (ci, [vp, ci, cu, cu, ci, cu, cu, vp, sz, vp]),
        "qoimi_hash_streams": (ci, [vp, vp, sz, vp, ci, vp, vp]),
        "qoimi_workspace_bytes": (None, [vp, szp]),
        "qoimi_set_decode_record_cap": (ci, [vp, sz, ci]),
        "qoimi_decode_stats": stats,
        "qoimi_set_profiling": (ci, [vp, ci]),
        "qoimi_get_profile": (ci, [vp, vp, P(ctypes.c_double), llp, ci]),
        "qoimi_kernel_name": (cs, [ci]),
        "qoimi_version": (cs, []),
    }


# name -> (restype, argtypes) of every function the header declares, in the header's order
PROTOTYPES = _prototypes()
