// PCM decode: the `data` chunk of a little-endian RIFF/WAVE file -> the mono fp32 waveform (include/beat_this_amd.h, "PCM
// decode": the arithmetic contract).  What preprocessing.load_audio + signal.mean(1) + the fp32 conversion do on the host in
// float64 -- 365 ms for a 5-minute stereo file in front of 5 ms of device work -- as one streaming kernel over the bytes as
// they lie in the file.
//
// Kernel shape.  A thread produces BT_PCM_THREAD_FRAMES = 4 consecutive output samples and writes them with one 16-byte store.
// The 4 C bytes_per_sample source bytes it needs are a whole number of dwords (C bytes_per_sample of them) at ANY byte phase:
// it reads the aligned dwords that enclose them (C bytes_per_sample + 1; the compiler merges them into dwordx4 / x3 / x2
// loads), turns them into the unaligned dwords with one byte-funnel shift each (v_alignbyte_b32), and cuts the samples out of
// those registers with shifts whose amounts are compile-time constants -- the kernel is instantiated per (format, channels),
// and a workgroup branches once, uniformly, to its track's instantiation.  No byte-wise loads on this path: a 24-bit stereo
// frame at an odd phase costs the same shifts as any other.  A track's last thread (fewer than 4 frames left) reads only the
// dwords that hold payload bytes and stores its samples one by one.
// fp64 work per output sample: C conversions, C adds, one division (a power-of-two C divides exactly like any other: IEEE).
// Built with -ffp-contract=off (_lib.FLAGS_BY_SOURCE): no multiply-add contraction anywhere in it.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/beat_this_amd.h"

#pragma clang fp contract(off)

int bt_set_error_external(int code, const char* msg);   // engine.hip (bt_last_error)

namespace {

#define HD __host__ __device__ __forceinline__

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int THREADS = BT_PCM_BLOCK_FRAMES / BT_PCM_THREAD_FRAMES;

HD constexpr int sample_bytes(int fmt) { return fmt == BT_PCM_U8 ? 1 : fmt == BT_PCM_S16 ? 2 : fmt == BT_PCM_S24 ? 3 : fmt == BT_PCM_F64 ? 8 : 4; }

HD bool format_ok(int fmt, int ch) {
  if (fmt < BT_PCM_U8 || fmt > BT_PCM_F64 || ch < 1) return false;
  return ch <= (fmt >= BT_PCM_F32 ? BT_PCM_MAX_CHANNELS_FLOAT : BT_PCM_MAX_CHANNELS_INT);
}

// ---- the arithmetic, shared by the kernel and the host twin ---------------------------------------------------------------
// the exact value of one sample from its little-endian bits (the low sample_bytes(FMT) bytes of ``bits``; the rest is ignored)
template <int FMT> HD double sample_value(uint64_t bits) {
  if (FMT == BT_PCM_U8) return (double)((int)(bits & 0xFF) - 128) * (1.0 / 128.0);
  if (FMT == BT_PCM_S16) return (double)(int16_t)(uint16_t)bits * (1.0 / 32768.0);
  if (FMT == BT_PCM_S24) return (double)((int32_t)((uint32_t)bits << 8) >> 8) * (1.0 / 8388608.0);
  if (FMT == BT_PCM_S32) return (double)(int32_t)(uint32_t)bits * (1.0 / 2147483648.0);
  if (FMT == BT_PCM_F32) {
    const uint32_t u = (uint32_t)bits;
    float f;
    memcpy(&f, &u, 4);
    return (double)f;
  }
  double d;
  memcpy(&d, &bits, 8);
  return d;
}

// one output sample from the C samples of a frame: ``bits(c)`` -> the bits of channel c
template <int FMT, int C, typename Bits> HD float frame_value(Bits bits) {
  if (C == 1) {
    if (FMT == BT_PCM_F32) {   // the sample itself
      const uint32_t u = (uint32_t)bits(0);
      float f;
      memcpy(&f, &u, 4);
      return f;
    }
    return (float)sample_value<FMT>(bits(0));
  }
  double acc = 0.0 + sample_value<FMT>(bits(0));   // (numpy's row sum starts at +0.0: -0.0 in every channel gives +0.0)
#pragma unroll
  for (int c = 1; c < C; ++c) acc = acc + sample_value<FMT>(bits(c));
  acc = acc / (double)C;
  return (float)acc;
}

struct Span { const uint8_t* src; long n; float* out; int fmt, ch; };
static_assert(sizeof(Span) == sizeof(bt_pcm_span), "bt_pcm_span layout");

// ---- device ---------------------------------------------------------------------------------------------------------------
#define DEVI __device__ __forceinline__
#define GLOBAL __attribute__((address_space(1)))   // the table hands out plain pointers: say that they are global, not flat

// frames [f0, f0 + nf) of a track, nf in 1 .. 4, f0 a multiple of 4
template <int FMT, int C> DEVI void decode_thread(const uint8_t* src, long f0, int nf, float* out) {
  constexpr int BPS = sample_bytes(FMT), FB = C * BPS;
  constexpr int ND = FB;                       // dwords in 4 frames: 4 FB / 4
  const uintptr_t s = (uintptr_t)src + (uintptr_t)f0 * FB;
  const GLOBAL uint32_t* a = (const GLOBAL uint32_t*)(s & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(s & 3);
  uint32_t r[ND + 1];
  if (nf == BT_PCM_THREAD_FRAMES) {
#pragma unroll
    for (int k = 0; k < ND; ++k) r[k] = a[k];
    r[ND] = sh ? a[ND] : 0u;                   // (phase 0: that dword holds no byte of these frames, and may lie past the payload's window)
  } else {
    const int nb = (int)sh + nf * FB;          // bytes from ``a`` to the end of the track
#pragma unroll
    for (int k = 0; k <= ND; ++k) r[k] = 4 * k < nb ? a[k] : 0u;
  }
  uint32_t w[ND];                              // the 4 frames' bytes as dwords: the 64-bit pair (r[k+1], r[k]) >> 8 sh
#pragma unroll
  for (int k = 0; k < ND; ++k) w[k] = __builtin_amdgcn_alignbyte(r[k + 1], r[k], sh);
  float v[BT_PCM_THREAD_FRAMES];
#pragma unroll
  for (int j = 0; j < BT_PCM_THREAD_FRAMES; ++j) {
    v[j] = frame_value<FMT, C>([&](int c) -> uint64_t {
      const int o = (j * C + c) * BPS, i = o >> 2, p = o & 3;   // (constants after unrolling)
      if constexpr (BPS == 8) return (uint64_t)w[i] | ((uint64_t)w[i + 1] << 32);
      if (p + BPS <= 4) return (uint64_t)(w[i] >> (8 * p));
      return (uint64_t)((w[i] >> (8 * p)) | (w[(i + 1) % ND] << ((32 - 8 * p) & 31)));   // a 24-bit sample across two dwords (% and &: the untaken instantiations stay in range)
    });
  }
  GLOBAL float* o = (GLOBAL float*)(uintptr_t)(out + f0);
  if (nf == BT_PCM_THREAD_FRAMES) {
    *(GLOBAL f32x4*)o = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < BT_PCM_THREAD_FRAMES - 1; ++j)
      if (j < nf) o[j] = v[j];
  }
}

template <int FMT> DEVI void decode_format(const Span& t, long f0, int nf) {
  switch (t.ch) {
    case 1: decode_thread<FMT, 1>(t.src, f0, nf, t.out); break;
    case 2: decode_thread<FMT, 2>(t.src, f0, nf, t.out); break;
    case 3: decode_thread<FMT, 3>(t.src, f0, nf, t.out); break;
    case 4: decode_thread<FMT, 4>(t.src, f0, nf, t.out); break;
    case 5: decode_thread<FMT, 5>(t.src, f0, nf, t.out); break;
    case 6: decode_thread<FMT, 6>(t.src, f0, nf, t.out); break;
    case 7: decode_thread<FMT, 7>(t.src, f0, nf, t.out); break;
    case 8:
      if (FMT < BT_PCM_F32) decode_thread<FMT, FMT < BT_PCM_F32 ? 8 : 1>(t.src, f0, nf, t.out);
      break;
    default: break;
  }
}

// grid (blocks of BT_PCM_BLOCK_FRAMES frames over the longest track, tracks); ``tracks`` null: the one track ``one``.
// A table entry outside the contract (format, channels, a null pointer) writes nothing.
__global__ __launch_bounds__(THREADS) void pcm_decode_kernel(Span one, const Span* __restrict__ tracks) {
  const Span t = tracks ? tracks[blockIdx.y] : one;
  const long f0 = ((long)blockIdx.x * THREADS + threadIdx.x) * BT_PCM_THREAD_FRAMES;
  if (f0 >= t.n || !t.src || !t.out) return;
  const long left = t.n - f0;
  const int nf = left < BT_PCM_THREAD_FRAMES ? (int)left : BT_PCM_THREAD_FRAMES;
  switch (t.fmt) {
    case BT_PCM_U8: decode_format<BT_PCM_U8>(t, f0, nf); break;
    case BT_PCM_S16: decode_format<BT_PCM_S16>(t, f0, nf); break;
    case BT_PCM_S24: decode_format<BT_PCM_S24>(t, f0, nf); break;
    case BT_PCM_S32: decode_format<BT_PCM_S32>(t, f0, nf); break;
    case BT_PCM_F32: decode_format<BT_PCM_F32>(t, f0, nf); break;
    case BT_PCM_F64: decode_format<BT_PCM_F64>(t, f0, nf); break;
    default: break;
  }
}

// ---- host twin ------------------------------------------------------------------------------------------------------------
template <int FMT, int C> void decode_host(const uint8_t* src, long n, float* out) {
  constexpr int BPS = sample_bytes(FMT);
  for (long f = 0; f < n; ++f) {
    const uint8_t* p = src + (size_t)f * C * BPS;
    out[f] = frame_value<FMT, C>([&](int c) -> uint64_t {
      uint64_t bits = 0;
      memcpy(&bits, p + c * BPS, BPS);   // (little-endian host)
      return bits;
    });
  }
}

template <int FMT> void decode_host_format(const uint8_t* src, int ch, long n, float* out) {
  switch (ch) {
    case 1: decode_host<FMT, 1>(src, n, out); break;
    case 2: decode_host<FMT, 2>(src, n, out); break;
    case 3: decode_host<FMT, 3>(src, n, out); break;
    case 4: decode_host<FMT, 4>(src, n, out); break;
    case 5: decode_host<FMT, 5>(src, n, out); break;
    case 6: decode_host<FMT, 6>(src, n, out); break;
    case 7: decode_host<FMT, 7>(src, n, out); break;
    case 8: decode_host<FMT, 8>(src, n, out); break;
    default: break;
  }
}

int fail(const char* fn, const char* msg, int code = BT_ERR_ARG) {
  return bt_set_error_external(code, (std::string(fn) + ": " + msg).c_str());
}

int launch(const char* fn, hipStream_t st, const Span& one, const Span* d_tracks, int n_tracks, int64_t max_frames) {
  if (max_frames == 0) return BT_OK;   // (nothing to write)
  const int64_t blocks = (max_frames + BT_PCM_BLOCK_FRAMES - 1) / BT_PCM_BLOCK_FRAMES;
  if (blocks > 0x7FFFFFFFll) return fail(fn, "too many frames for one launch");
  hipLaunchKernelGGL(pcm_decode_kernel, dim3((unsigned)blocks, (unsigned)n_tracks), dim3(THREADS), 0, st, one, d_tracks);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? BT_OK : fail(fn, hipGetErrorString(e), BT_ERR_HIP);
}

}  // namespace

extern "C" {

int bt_pcm_decode_batch(void* stream, const bt_pcm_span* d_tracks, int n_tracks, int64_t max_frames) {
  const char* fn = "bt_pcm_decode_batch";
  if (!d_tracks) return fail(fn, "null argument");
  if (n_tracks < 0 || max_frames < 0) return fail(fn, "negative count");
  if (n_tracks > BT_PCM_MAX_TRACKS) return fail(fn, "more than BT_PCM_MAX_TRACKS tracks");
  if (n_tracks == 0) return BT_OK;
  return launch(fn, (hipStream_t)stream, Span{nullptr, 0, nullptr, 0, 0}, reinterpret_cast<const Span*>(d_tracks), n_tracks, max_frames);
}

int bt_pcm_decode(void* stream, const uint8_t* d_src, int format, int channels, int64_t n_frames, float* d_out) {
  const char* fn = "bt_pcm_decode";
  if (!d_src || !d_out) return fail(fn, "null argument");
  if (!format_ok(format, channels)) return fail(fn, "unknown format, or a channel count outside 1 .. 8 (integer) / 1 .. 7 (float)");
  if (n_frames < 0) return fail(fn, "negative count");
  if ((uintptr_t)d_out & 15) return fail(fn, "d_out must be 16-byte aligned");
  return launch(fn, (hipStream_t)stream, Span{d_src, (long)n_frames, d_out, format, channels}, nullptr, 1, n_frames);
}

int bt_pcm_decode_host(const uint8_t* src, int format, int channels, int64_t n_frames, float* out) {
  const char* fn = "bt_pcm_decode_host";
  if (!src || !out) return fail(fn, "null argument");
  if (!format_ok(format, channels)) return fail(fn, "unknown format, or a channel count outside 1 .. 8 (integer) / 1 .. 7 (float)");
  if (n_frames < 0) return fail(fn, "negative count");
  switch (format) {
    case BT_PCM_U8: decode_host_format<BT_PCM_U8>(src, channels, (long)n_frames, out); break;
    case BT_PCM_S16: decode_host_format<BT_PCM_S16>(src, channels, (long)n_frames, out); break;
    case BT_PCM_S24: decode_host_format<BT_PCM_S24>(src, channels, (long)n_frames, out); break;
    case BT_PCM_S32: decode_host_format<BT_PCM_S32>(src, channels, (long)n_frames, out); break;
    case BT_PCM_F32: decode_host_format<BT_PCM_F32>(src, channels, (long)n_frames, out); break;
    default: decode_host_format<BT_PCM_F64>(src, channels, (long)n_frames, out); break;
  }
  return BT_OK;
}

}  // extern "C"
