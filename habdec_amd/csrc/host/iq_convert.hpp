// Packed IQ sample formats (include/habdec_amd.h: HD_IQ_*) on the host: bytes per sample and the conversion to interleaved float32 that
// kernels/iq_unpack.hip performs on the GPU.  Little-endian, I then Q:
//
//   cs16: (float)v * 2^-15      cs8: (float)v * 2^-7      cu8: (float)(2 v - 255) * 2^-8   (centre 127.5: 0 -> -255/256, 255 -> +255/256)
//
// Every value is an integer of at most 16 bits times a power of two, so it is exact in float and the kernel agrees with this model bit for bit.
// The bytes are read one at a time: no alignment is asked of `src`, and nothing outside [src, src + n * bps) is touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstring>

#include "../../../include/habdec_amd.h"

namespace hd {

inline constexpr size_t iq_bytes(int fmt)      // bytes per complex sample; 0 = unknown format
{
    return fmt == HD_IQ_CF32 ? 8u : fmt == HD_IQ_CS16 ? 4u : (fmt == HD_IQ_CS8 || fmt == HD_IQ_CU8) ? 2u : 0u;
}

inline void iq_convert(int fmt, const void* src, size_t n, float* out)     // n complex samples -> 2 n floats; an unknown format writes nothing
{
    const unsigned char* p = static_cast<const unsigned char*>(src);
    switch (fmt) {
    case HD_IQ_CF32: std::memcpy(out, src, n * 8u); break;
    case HD_IQ_CS16:
        for (size_t i = 0; i < 2 * n; ++i) out[i] = (float)(int16_t)(uint16_t)(p[2 * i] | (p[2 * i + 1] << 8)) * 0x1p-15f;
        break;
    case HD_IQ_CS8:
        for (size_t i = 0; i < 2 * n; ++i) out[i] = (float)(int8_t)p[i] * 0x1p-7f;
        break;
    case HD_IQ_CU8:
        for (size_t i = 0; i < 2 * n; ++i) out[i] = (float)(2 * (int)p[i] - 255) * 0x1p-8f;
        break;
    default: break;
    }
}

}  // namespace hd
