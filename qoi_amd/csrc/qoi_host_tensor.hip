// qoi_host_tensor.hip — the tensor calls of the C-ABI shim: qoimi_decode_tensors (the area filter, the antialiased bilinear filter or the
// antialiased bicubic and Lanczos filters, the nearest filter and the mode filter, which only this call has) and qoimi_decode_warped_tensors, with qoimi_tensor_size and qoimi_warp_tensor_size.  They are gather_resampled and gather_warped of qoi_staged.h -
// the checks of the items, the plan, the table entries and run_staged of qoimi_decode_resized / _bilinear / _warped - with the checks of the
// format in front, output sizes in bytes of elements, the alignment of the outputs behind, and the tensor kernels of qoi_tensor.hip as the
// launch.
#include "qoi_staged.h"
#include "qoi_lanczos_core.h"
#include "qoi_mode_core.h"
#include "qoi_nearest_core.h"
#include "qoi_tensor_core.h"

#include <math.h>
#include <stddef.h>

static_assert(sizeof(qoimi_tensor_format) == 48 && offsetof(qoimi_tensor_format, dtype) == 0 && offsetof(qoimi_tensor_format, layout) == 4 &&
              offsetof(qoimi_tensor_format, scale) == 8 && offsetof(qoimi_tensor_format, bias) == 24 && offsetof(qoimi_tensor_format, reserved) == 40,
              "qoimi_tensor_format layout");
static_assert(sizeof(TensorFormat) == 40, "the format is ten dwords of kernel arguments");
static_assert(QOIMI_TENSOR_U8 == (int)kTensorU8 && QOIMI_TENSOR_F16 == (int)kTensorF16 && QOIMI_TENSOR_BF16 == (int)kTensorBF16 && QOIMI_TENSOR_F32 == (int)kTensorF32 &&
              QOIMI_TENSOR_I32 == (int)kTensorI32 && QOIMI_TENSOR_I64 == (int)kTensorI64 &&
              QOIMI_TENSOR_HWC == (int)kTensorHWC && QOIMI_TENSOR_CHW == (int)kTensorCHW && QOIMI_TENSOR_HW == (int)kTensorHW, "the kernels take dtype and layout as numbers");
static_assert(QOIMI_TENSOR_I32 == 5 && QOIMI_TENSOR_I64 == 6 && QOIMI_TENSOR_HW == 3, "4 is not a dtype, 2 is not a layout");
static_assert(QOIMI_TENSOR_HW_ID24 == (int)kTensorHWId24 && QOIMI_TENSOR_HW_ID24 == 5, "the id layout; 4 is not a layout");

static bool tensor_dtype_known(unsigned dtype) { return dtype <= (unsigned)QOIMI_TENSOR_F32 || dtype == (unsigned)QOIMI_TENSOR_I32 || dtype == (unsigned)QOIMI_TENSOR_I64; }
static bool tensor_layout_known(unsigned layout) { return layout <= (unsigned)QOIMI_TENSOR_CHW || layout == (unsigned)QOIMI_TENSOR_HW || layout == (unsigned)QOIMI_TENSOR_HW_ID24; }

// nullptr if the format is fine, else what is wrong with it - in the order the header gives
static const char* tensor_format_wrong(const qoimi_tensor_format* f) {
    if (!f) return "format is NULL";
    if (!tensor_dtype_known(f->dtype)) return "unknown dtype";
    if (!tensor_layout_known(f->layout)) return "unknown layout";
    if (f->reserved[0] != 0u || f->reserved[1] != 0u) return "format reserved is not 0";
    for (int k = 0; k < 4; ++k) {
        if (!isfinite(f->scale[k]) || !isfinite(f->bias[k])) return "scale or bias is not finite";
    }
    if (tensor_integer(f->dtype)) {                                // (the element is the byte's value: nothing is scaled)
        for (int k = 0; k < 4; ++k) {
            if (f->scale[k] != 1.0f || f->bias[k] != 0.0f || signbit(f->bias[k]))
                return f->dtype == (unsigned)QOIMI_TENSOR_U8 ? "QOIMI_TENSOR_U8 takes scale 1 and bias +0 only"
                     : f->dtype == (unsigned)QOIMI_TENSOR_I32 ? "QOIMI_TENSOR_I32 takes scale 1 and bias +0 only" : "QOIMI_TENSOR_I64 takes scale 1 and bias +0 only";
        }
    }
    if (f->layout == (unsigned)QOIMI_TENSOR_HW_ID24 && f->dtype != (unsigned)QOIMI_TENSOR_I32 && f->dtype != (unsigned)QOIMI_TENSOR_I64)
        return "QOIMI_TENSOR_HW_ID24 takes QOIMI_TENSOR_I32 or QOIMI_TENSOR_I64 only (an id does not fit a byte, and is not scaled)";
    return nullptr;
}

static int check_tensor_format(const qoimi_tensor_format* f) {
    if (const char* what = tensor_format_wrong(f)) return fail(QOIMI_E_ARG, what);
    return QOIMI_OK;
}

static TensorFormat kernel_format(const qoimi_tensor_format* f) {
    TensorFormat t;
    t.dtype = f->dtype; t.layout = f->layout;
    for (int k = 0; k < 4; ++k) { t.scale[k] = f->scale[k]; t.bias[k] = f->bias[k]; }
    return t;
}

// Bytes of an element of the format; 1 for a format the check rejects (used behind the format's check only)
static size_t format_elem(const qoimi_tensor_format* f) { return (f && tensor_dtype_known(f->dtype)) ? tensor_elem(f->dtype) : 1u; }
// Elements of a pixel of an output with och channels: one under QOIMI_TENSOR_HW and QOIMI_TENSOR_HW_ID24
static unsigned format_channels(const qoimi_tensor_format* f, unsigned och) {
    return (f && (f->layout == (unsigned)QOIMI_TENSOR_HW || f->layout == (unsigned)QOIMI_TENSOR_HW_ID24)) ? 1u : och;
}

// pixel_bytes (resize_bytes, warp_bytes: the u8 output) at the format's elements per pixel times the element size, false if that does not
// fit a size_t
template <class Item>
static bool tensor_bytes(bool (*pixel_bytes)(const Item*, unsigned, size_t*), const Item* r, unsigned och, const qoimi_tensor_format* f, size_t* bytes) {
    size_t b = 0;
    const size_t elem = format_elem(f);
    if (!pixel_bytes(r, format_channels(f, och), &b) || b > ~(size_t)0 / elem) return false;
    *bytes = b * elem;
    return true;
}

// Every output begins at a multiple of the element size
static int check_tensor_alignment(const void* d_out, const size_t* out_offsets, size_t n, size_t elem) {
    for (size_t j = 0; j < n; ++j) {
        if (((uintptr_t)d_out + out_offsets[j]) % elem != 0u)
            return fail(QOIMI_E_ARG, "item " + std::to_string(j) + ": the output address is not a multiple of the element size");
    }
    return QOIMI_OK;
}

static_assert(QOIMI_FILTER_AREA == 0 && QOIMI_FILTER_BILINEAR == 1 && QOIMI_FILTER_BICUBIC == 3 && QOIMI_FILTER_LANCZOS == 6 && QOIMI_FILTER_NEAREST == 9 &&
              QOIMI_FILTER_MODE == 11, "2, 4, 5, 7 and 8 are not filters, nor is 10");
static_assert(kNearestMaxSize == kCubicMaxSize, "the nearest filter has the bicubic filter's size limit");
static_assert(kLanczosMaxRatio == kCubicMaxRatio && kLanczosMaxSize == kCubicMaxSize, "the two filters share their limits: cubic_item_wrong");

// ... with the ratio limit of 16 and the size limit (qoi_cubic_core.h, qoi_lanczos_core.h: what keeps the weights in 64 bits and a tile's tables
// in their LDS)
static const char* cubic_item_wrong(const qoi_desc* d, const qoimi_resize* r) {
    if (const char* what = resample_rect_wrong(d, r)) return what;
    if (r->width > (uint64_t)kCubicMaxRatio * r->out_width || r->height > (uint64_t)kCubicMaxRatio * r->out_height) return "reduced by more than 16 in an axis";
    if (r->width > kCubicMaxSize || r->out_width > kCubicMaxSize || r->height > kCubicMaxSize || r->out_height > kCubicMaxSize) return "a width or height above 16384";
    return nullptr;
}

// ... with the size limit alone (qoi_nearest_core.h: what keeps an index in one 32-bit division): no ratio limit, every output pixel is one load
static const char* nearest_item_wrong(const qoi_desc* d, const qoimi_resize* r) {
    if (const char* what = resample_rect_wrong(d, r)) return what;
    if (r->width > kNearestMaxSize || r->out_width > kNearestMaxSize || r->height > kNearestMaxSize || r->out_height > kNearestMaxSize) return "a width or height above 16384";
    return nullptr;
}

// ... with a ratio limit of 16 and the size limit (qoi_mode_core.h: what keeps a cell within 16 x 16 pixels - four a lane of a wavefront - and
// its ends in one 32-bit division each)
static const char* mode_item_wrong(const qoi_desc* d, const qoimi_resize* r) {
    if (const char* what = resample_rect_wrong(d, r)) return what;
    if (r->width > (uint64_t)kModeMaxRatio * r->out_width || r->height > (uint64_t)kModeMaxRatio * r->out_height) return "reduced by more than 16 in an axis";
    if (r->width > kModeMaxSize || r->out_width > kModeMaxSize || r->height > kModeMaxSize || r->out_height > kModeMaxSize) return "a width or height above 16384";
    return nullptr;
}

// The bicubic, the Lanczos, the nearest and the mode filter write tensors only: no launcher of a byte kernel, the counters and the name are the tensor call's.
static const ResampleKind kCubicKind = {cubic_item_wrong, split_columns<cubic_split>, tiles_columns<cubic_tiles>, nullptr, &qoimi_ctx::tensor_stats, "tensor_cubic"};
static const ResampleKind kLanczosKind = {cubic_item_wrong, split_columns<lanczos_split>, tiles_columns<lanczos_tiles>, nullptr, &qoimi_ctx::tensor_stats, "tensor_lanczos"};
static const ResampleKind kNearestKind = {nearest_item_wrong, split_columns<nearest_split>, tiles_columns<nearest_tiles>, nullptr, &qoimi_ctx::tensor_stats, "tensor_nearest"};
static const ResampleKind kModeKind = {mode_item_wrong, mode_split, mode_tiles, nullptr, &qoimi_ctx::tensor_stats, "tensor_mode"};

// A filter of qoimi_decode_tensors: its kind, the launcher of its tensor kernel and that kernel's name for a launch failure
struct TensorFilter {
    const ResampleKind* kind;
    void (*launch)(const uint8_t*, const ResizeEntry*, uint32_t, uint32_t, uint8_t*, const TensorFormat&, uint32_t, hipStream_t);
    const char* kernel;
};

static TensorFilter tensor_filter(int filter) {
    switch (filter) {
    case QOIMI_FILTER_AREA: return {&kAreaKind, launch_tensor_area, "tensor_area"};
    case QOIMI_FILTER_BILINEAR: return {&kTentKind, launch_tensor_tent, "tensor_tent"};
    case QOIMI_FILTER_BICUBIC: return {&kCubicKind, launch_tensor_cubic, kCubicKind.kernel};
    case QOIMI_FILTER_LANCZOS: return {&kLanczosKind, launch_tensor_lanczos, kLanczosKind.kernel};
    case QOIMI_FILTER_NEAREST: return {&kNearestKind, launch_tensor_nearest, kNearestKind.kernel};
    case QOIMI_FILTER_MODE: return {&kModeKind, launch_tensor_mode, kModeKind.kernel};
    default: return {nullptr, nullptr, nullptr};
    }
}

extern "C" size_t qoimi_tensor_size(const qoi_desc* desc, const qoimi_resize* item, int filter, int channels, const qoimi_tensor_format* format) {
    const ResampleKind* kind = tensor_filter(filter).kind;
    size_t bytes = 0;
    if (!kind || !desc_ok(desc) || !item || (channels != 3 && channels != 4) || tensor_format_wrong(format) || kind->wrong(desc, item) ||
        !tensor_bytes(resize_bytes, item, (unsigned)channels, format, &bytes)) return 0;
    return bytes;
}

extern "C" size_t qoimi_warp_tensor_size(const qoi_desc* desc, const qoimi_warp* item, int channels, const qoimi_tensor_format* format) {
    size_t bytes = 0;
    if (!desc_ok(desc) || !item || (channels != 3 && channels != 4) || tensor_format_wrong(format) || warp_item_wrong(desc, item) ||
        !tensor_bytes(warp_bytes, item, (unsigned)channels, format, &bytes)) return 0;
    return bytes;
}

extern "C" int qoimi_decode_tensors(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                    int n_images, int channels, const qoimi_resize* items, int n_items, int filter, int mode,
                                    const qoimi_tensor_format* format, void* d_out, const size_t* out_offsets, size_t staging_bytes, void* stream) {
    const TensorFilter tf = tensor_filter(filter);
    if (!tf.kind) return fail(QOIMI_E_ARG, "filter must be QOIMI_FILTER_LANCZOS, QOIMI_FILTER_AREA, QOIMI_FILTER_BILINEAR or QOIMI_FILTER_BICUBIC, or QOIMI_FILTER_NEAREST or QOIMI_FILTER_MODE");
    return gather_resampled(*tf.kind, c, d_streams, stream_offsets, sizes, descs, n_images, channels, items, n_items, mode, d_out, out_offsets, staging_bytes, stream,
        [&]() { return check_tensor_format(format); },
        [&](const qoimi_resize* r, unsigned och, size_t* bytes) { return tensor_bytes(resize_bytes, r, och, format, bytes); },
        [&](const CheckedItems&) { return check_tensor_alignment(d_out, out_offsets, (size_t)n_items, format_elem(format)); },
        &qoimi_ctx::tensor_stats, tf.kernel,
        [&](const ResizeEntry* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) {
            tf.launch((const uint8_t*)c->ver_stage.base, tab, m, tiles, (uint8_t*)d_out, kernel_format(format), grid, st);
        });
}

extern "C" int qoimi_decode_warped_tensors(qoimi_ctx* c, const void* d_streams, const size_t* stream_offsets, const int* sizes, const qoi_desc* descs,
                                           int n_images, int channels, const qoimi_warp* items, int n_items, int mode,
                                           const qoimi_tensor_format* format, void* d_out, const size_t* out_offsets, size_t staging_bytes, void* stream) {
    return gather_warped(c, d_streams, stream_offsets, sizes, descs, n_images, channels, items, n_items, mode, d_out, out_offsets, staging_bytes, stream,
        [&]() { return check_tensor_format(format); },
        [&](const qoimi_warp* r, unsigned och, size_t* bytes) { return tensor_bytes(warp_bytes, r, och, format, bytes); },
        [&](const CheckedItems&) { return check_tensor_alignment(d_out, out_offsets, (size_t)n_items, format_elem(format)); },
        &qoimi_ctx::tensor_stats, {"tensor_warp", "warp_bicubic_tensor", "warp_border_tensor", "warp_super_tensor", "warp_vote_tensor"}, "warp_proj_tensor",
        [&](WarpKernel kind, const WarpEntry* tab, uint32_t m, uint32_t tiles, uint32_t grid, hipStream_t st) {
            (kind == kWarpKernelProj ? launch_tensor_warp_proj : kind == kWarpKernelVote ? launch_tensor_warp_vote
                                     : (kind == kWarpKernelSuper ? launch_tensor_warp_super
                                     : (kind == kWarpKernelBorder ? launch_tensor_warp_border : (kind == kWarpKernelCubic ? launch_tensor_warp_cubic : launch_tensor_warp))))(
                (const uint8_t*)c->ver_stage.base, tab, m, tiles, (uint8_t*)d_out, kernel_format(format), grid, st);
        });
}
