// host_sink.h — the TensorSink of a call's format, for the host harnesses that write tensors (beside host_mem.h, which the harnesses that write
// bytes only use alone).  Not part of the library.
#pragma once
#include "../../qoi_amd/csrc/qoi_tensor_core.h"

namespace hostmem {

inline qoimi::TensorSink tensor_sink(uint32_t dtype, uint32_t layout, const float* scale, const float* bias) {
    qoimi::TensorSink sink;
    sink.fmt.dtype = dtype; sink.fmt.layout = layout;
    for (int k = 0; k < 4; ++k) { sink.fmt.scale[k] = scale[k]; sink.fmt.bias[k] = bias[k]; }
    return sink;
}

// u8 HWC with scale 1 and bias 0: what the byte-writing filter kernels pass
inline qoimi::TensorSink tensor_sink_u8_hwc() {
    const float one[4] = {1.0f, 1.0f, 1.0f, 1.0f}, zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    return tensor_sink(qoimi::kTensorU8, qoimi::kTensorHWC, one, zero);
}

}  // namespace hostmem
