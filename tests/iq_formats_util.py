"""Shared by the packed-IQ tests (test_iq_formats_host.py, test_gpu_iq_formats.py): the formats, the conversion through the library's host model
(hd_host_iq_convert) and the quantiser that makes packed test inputs out of synthetic floats."""
import numpy as np

# name -> (HD_IQ_*, dtype of one component, bytes per complex sample)
FMTS = {"cs16": (1, np.dtype("<i2"), 4), "cs8": (2, np.dtype(np.int8), 2), "cu8": (3, np.dtype(np.uint8), 2)}


def convert(fmt: str, packed: np.ndarray) -> np.ndarray:
    """Packed samples [..., 2] -> complex64 [...] through hd_host_iq_convert."""
    import habdec_amd
    code, dt, _ = FMTS[fmt]
    packed = np.ascontiguousarray(packed, dtype=dt)
    assert packed.shape[-1] == 2
    out = np.zeros(packed.size, np.float32)
    habdec_amd.lib().hd_host_iq_convert(code, packed.ctypes.data, packed.size // 2, out)
    return out.view(np.complex64).reshape(packed.shape[:-1])


def model(fmt: str, packed: np.ndarray) -> np.ndarray:
    """The issue's table in float64, then cast: float32 [..., 2]."""
    v = np.asarray(packed).astype(np.float64)
    if fmt == "cs16":
        return (v * 2.0 ** -15).astype(np.float32)
    if fmt == "cs8":
        return (v * 2.0 ** -7).astype(np.float32)
    return ((2.0 * v - 255.0) * 2.0 ** -8).astype(np.float32)


def quantise(fmt: str, iq: np.ndarray) -> np.ndarray:
    """complex64 [...] with |component| < 1 -> packed [..., 2], rounded to the nearest code (full scale = 1.0: a synth signal of amplitude 0.5
    sits at half of full scale)."""
    x = np.stack([iq.real, iq.imag], axis=-1).astype(np.float64)
    if fmt == "cs16":
        return np.clip(np.rint(x * 32768.0), -32768, 32767).astype("<i2")
    if fmt == "cs8":
        return np.clip(np.rint(x * 128.0), -128, 127).astype(np.int8)
    return np.clip(np.rint((x * 256.0 + 255.0) / 2.0), 0, 255).astype(np.uint8)


def all_codes(fmt: str) -> np.ndarray:
    """[N, 2]: every code of the format in I (beside a running Q) and in Q (beside a running I)."""
    _, dt, _ = FMTS[fmt]
    info = np.iinfo(dt)
    codes = np.arange(info.min, info.max + 1, dtype=np.int64)
    other = codes[::-1]
    a = np.stack([codes, (other * 7 + 3 - info.min) % (info.max - info.min + 1) + info.min], axis=-1)
    b = np.stack([(other * 5 + 1 - info.min) % (info.max - info.min + 1) + info.min, codes], axis=-1)
    return np.concatenate([a, b]).astype(dt)
