// FLAC decode: a FLAC file's bytes -> the mono fp32 waveform (include/beat_this_amd.h, "FLAC decode": the contract).  The
// bit reader, the header parser and the subframe walker are csrc/flac_bits.h, one text for the kernels and the host twin.
//
// A FLAC frame has no length field, so finding the frames is part of the decode and happens here, on the device; the host
// reads the metadata blocks only.  Seven launches per call, whatever the number of tracks (blockIdx.y = track, a device
// table of spans as in pcm.hip):
//   scan     one thread per byte offset from first_frame on: is this a frame header of this stream?  -> a count per
//            workgroup of BT_FLAC_SCAN_BYTES offsets
//   prefix   one workgroup per track: the exclusive prefix sum of those counts (integers: no order dependence)
//   compact  the scan's test again, a ballot rank inside the workgroup -> the candidates' offsets in offset order
//   measure  one thread per candidate walks the frame's bits without storing a sample -> where it ends, or "not a frame"
//   link     one thread per track follows the chain from first_frame: each frame starts where the last one ended and
//            carries the next number; the chain ends exactly at total_samples -> the status, and each accepted frame's
//            sample position.  Only this step accepts a frame.
//   decode   one thread per accepted frame walks it again with a sink: residual -> predictor recurrence -> the planar
//            int32 workspace at the frame's true position, the stereo decorrelation undone as the second channel arrives.
//            LPC coefficients and the ring of the last 32 samples are LDS columns of the thread (no scratch).
//   mix      pcm.hip's channel mean over the planar integers, 4 output samples and one 16-byte store per thread.
// No atomics and no order that depends on scheduling: runs are bit-identical.
// Built with -ffp-contract=off (_lib.FLAGS_BY_SOURCE).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/beat_this_amd.h"
#include "flac_bits.h"

#pragma clang fp contract(off)

int bt_set_error_external(int code, const char* msg);   // engine.hip (bt_last_error)

namespace {

using flac::Info;

static_assert(sizeof(Info) == sizeof(bt_flac_info), "bt_flac_info layout");
static_assert(sizeof(flac::Status) == sizeof(bt_flac_status), "bt_flac_status layout");
static_assert(FL_OK == BT_FLAC_OK && FL_BROKEN == BT_FLAC_BROKEN && FL_LENGTH == BT_FLAC_LENGTH && FL_CANDIDATES == BT_FLAC_CANDIDATES, "status codes");

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr int SCAN = BT_FLAC_SCAN_BYTES;
constexpr int WALK = 64;                                   // threads per workgroup of measure / decode: one wave
constexpr int MIX_THREADS = BT_FLAC_BLOCK_SAMPLES / BT_FLAC_THREAD_SAMPLES;

struct Span { const uint8_t* src; float* out; void* ws; size_t ws_bytes; flac::Status* status; Info info; };
static_assert(sizeof(Span) == sizeof(bt_flac_span), "bt_flac_span layout");

struct Cand {            // 32 bytes
  int32_t off, end;      // end: the byte behind the frame, 0 = not a frame
  uint64_t num;
  int32_t block, assign;
  int64_t pos;           // first sample of an accepted frame, -1 otherwise
};

// one track's workspace: [planar int32: channels x ld][counts: nblk + 1 int32][candidates: cap x Cand]
struct Layout {
  int64_t ld, nblk, cap;
  size_t off_counts, off_cand, total;
};

__host__ __device__ __forceinline__ Layout layout(const Info& in) {
  Layout l;
  l.ld = (in.total_samples + 3) / 4 * 4;
  const int64_t span = in.n_bytes - in.first_frame;
  l.nblk = (span + SCAN - 1) / SCAN;
  l.cap = span / 8 + 64;
  l.off_counts = (size_t)in.channels * (size_t)l.ld * 4;
  l.off_cand = l.off_counts + ((size_t)(l.nblk + 1) * 4 + 15) / 16 * 16;
  l.total = l.off_cand + (size_t)l.cap * sizeof(Cand);
  return l;
}

bool info_ok(const Info& in, bool device) {
  if (in.channels < 1 || in.channels > 8 || in.bps < 4 || in.bps > 24 || in.sample_rate <= 0) return false;
  if (in.blocking < 0 || in.blocking > 1 || in.max_block < 1 || in.max_block > 65535 || in.total_samples <= 0) return false;
  if (in.first_frame < 0 || in.n_bytes <= 0 || in.first_frame >= in.n_bytes) return false;
  if (device && (in.n_bytes >= (1ll << 31) || in.total_samples >= (1ll << 31))) return false;
  return true;
}

// 4 consecutive output samples from the planar integers: quad(c) -> samples i .. i + 3 of channel c.  pcm.hip's arithmetic.
struct Quad { int32_t v[4]; };
template <class Load> __host__ __device__ __forceinline__ void mix4(Load quad, int channels, double scale, float* out) {
  double acc[4];
  {
    const Quad q = quad(0);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = channels == 1 ? (double)q.v[j] * scale : 0.0 + (double)q.v[j] * scale;
  }
  for (int c = 1; c < channels; ++c) {
    const Quad q = quad(c);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = acc[j] + (double)q.v[j] * scale;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = (float)(channels == 1 ? acc[j] : acc[j] / (double)channels);
}

// ---- device ---------------------------------------------------------------------------------------------------------------
#define DEVI __device__ __forceinline__

DEVI bool track_ok(const Span& t) { return t.src && t.out && t.ws && t.status; }
DEVI int32_t* counts_of(const Span& t, const Layout& l) { return (int32_t*)((char*)t.ws + l.off_counts); }
DEVI Cand* cands_of(const Span& t, const Layout& l) { return (Cand*)((char*)t.ws + l.off_cand); }

DEVI bool header_at(const Span& t, int64_t off, flac::Header& h) {
  return off < t.info.n_bytes && flac::parse_header(t.src, t.info.n_bytes, off, t.info, h);
}

__global__ __launch_bounds__(SCAN) void flac_scan_kernel(Span one, const Span* __restrict__ tracks) {
  const Span t = tracks ? tracks[blockIdx.y] : one;
  const Layout l = layout(t.info);
  if (!track_ok(t) || (int64_t)blockIdx.x >= l.nblk) return;
  flac::Header h;
  const int flag = header_at(t, t.info.first_frame + (int64_t)blockIdx.x * SCAN + threadIdx.x, h) ? 1 : 0;
  const int n = __syncthreads_count(flag);
  if (threadIdx.x == 0) counts_of(t, l)[blockIdx.x] = n;
}

// counts[0 .. nblk) -> their exclusive prefix sums, counts[nblk] = the total
__global__ __launch_bounds__(256) void flac_prefix_kernel(Span one, const Span* __restrict__ tracks) {
  const Span t = tracks ? tracks[blockIdx.y] : one;
  if (!track_ok(t)) return;
  const Layout l = layout(t.info);
  int32_t* counts = counts_of(t, l);
  __shared__ int32_t part[256];
  const int64_t seg = (l.nblk + 255) / 256;
  const int64_t a = (int64_t)threadIdx.x * seg, b = a + seg < l.nblk ? a + seg : l.nblk;
  int32_t sum = 0;
  for (int64_t i = a; i < b; ++i) sum += counts[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t run = 0;
    for (int i = 0; i < 256; ++i) {
      const int32_t v = part[i];
      part[i] = run;
      run += v;
    }
    counts[l.nblk] = run;
  }
  __syncthreads();
  int32_t run = part[threadIdx.x];
  for (int64_t i = a; i < b; ++i) {
    const int32_t v = counts[i];
    counts[i] = run;
    run += v;
  }
}

__global__ __launch_bounds__(SCAN) void flac_compact_kernel(Span one, const Span* __restrict__ tracks) {
  const Span t = tracks ? tracks[blockIdx.y] : one;
  const Layout l = layout(t.info);
  if (!track_ok(t) || (int64_t)blockIdx.x >= l.nblk) return;
  __shared__ int32_t wave_n[SCAN / 64];
  flac::Header h;
  const int64_t off = t.info.first_frame + (int64_t)blockIdx.x * SCAN + threadIdx.x;
  const bool flag = header_at(t, off, h);
  const uint64_t mask = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_n[wave] = __popcll(mask);
  __syncthreads();
  if (!flag) return;
  int64_t idx = counts_of(t, l)[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1));
  for (int w = 0; w < wave; ++w) idx += wave_n[w];
  if (idx < l.cap) cands_of(t, l)[idx].off = (int32_t)off;
}

DEVI int64_t n_cands(const Span& t, const Layout& l) {
  const int64_t n = counts_of(t, l)[l.nblk];
  return n < l.cap ? n : l.cap;
}

__global__ __launch_bounds__(WALK) void flac_measure_kernel(Span one, const Span* __restrict__ tracks) {
  const Span t = tracks ? tracks[blockIdx.y] : one;
  if (!track_ok(t)) return;
  const Layout l = layout(t.info);
  const int64_t i = (int64_t)blockIdx.x * WALK + threadIdx.x;
  if (i >= n_cands(t, l)) return;
  Cand* c = cands_of(t, l) + i;
  const int64_t off = c->off;
  flac::Header h;
  Cand r;
  r.off = (int32_t)off, r.end = 0, r.num = 0, r.block = 0, r.assign = 0, r.pos = -1;
  if (header_at(t, off, h)) {
    flac::NullSink sink;
    r.end = (int32_t)flac::walk_frame(t.src, t.info.n_bytes, off, t.info, h, sink, true);
    r.num = h.number, r.block = h.block, r.assign = h.assign;
  }
  *c = r;
}

__global__ __launch_bounds__(64) void flac_link_kernel(Span one, const Span* __restrict__ tracks) {
  const Span t = tracks ? tracks[blockIdx.y] : one;
  if (!track_ok(t) || threadIdx.x != 0) return;
  const Layout l = layout(t.info);
  Cand* cand = cands_of(t, l);
  const int64_t found = counts_of(t, l)[l.nblk], n = n_cands(t, l);
  int64_t p = t.info.first_frame, pos = 0, i = 0;
  int32_t frames = 0, code = FL_OK;
  uint64_t expect = 0;
  if (found > l.cap) {
    code = FL_CANDIDATES;
  } else {
    while (pos < t.info.total_samples) {
      while (i < n && cand[i].off < p) ++i;
      if (i >= n || cand[i].off != p || (frames > 0 && cand[i].num != expect)) {
        code = FL_BROKEN;
        break;
      }
      const int32_t block = cand[i].block, end = cand[i].end;
      if (pos + block > t.info.total_samples) {
        code = FL_LENGTH;
        break;
      }
      if (end == 0) {
        code = FL_BROKEN;
        break;
      }
      cand[i].pos = pos;
      expect = flac::next_number(t.info, cand[i].num, block);
      pos += block;
      p = end;
      ++frames;
    }
  }
  flac::Status s;
  s.code = code, s.n_frames = frames, s.n_samples = pos, s.where = p;
  *t.status = s;
}

struct LdsStore {
  int32_t* c;   // this thread's column of cf[32][WALK]
  int32_t* r;   // ... of ring[32][WALK]
  DEVI int32_t& cf(int j) { return c[j * WALK]; }
  DEVI int32_t& ring(int i) { return r[i * WALK]; }
};

__global__ __launch_bounds__(WALK) void flac_decode_kernel(Span one, const Span* __restrict__ tracks) {
  __shared__ int32_t cf[32 * WALK], ring[32 * WALK];
  const Span t = tracks ? tracks[blockIdx.y] : one;
  if (!track_ok(t) || t.status->code != FL_OK) return;
  const Layout l = layout(t.info);
  const int64_t i = (int64_t)blockIdx.x * WALK + threadIdx.x;
  if (i >= n_cands(t, l)) return;
  const Cand c = cands_of(t, l)[i];
  flac::Header h;
  if (c.pos < 0 || !header_at(t, c.off, h)) return;
  flac::PlanarSink<LdsStore> sink;
  sink.st.c = cf + threadIdx.x, sink.st.r = ring + threadIdx.x;
  sink.pl = (int32_t*)t.ws + c.pos, sink.ld = l.ld, sink.assign = h.assign;
  flac::walk_frame(t.src, t.info.n_bytes, c.off, t.info, h, sink, false);
}

__global__ __launch_bounds__(MIX_THREADS) void flac_mix_kernel(Span one, const Span* __restrict__ tracks) {
  const Span t = tracks ? tracks[blockIdx.y] : one;
  if (!track_ok(t) || t.status->code != FL_OK) return;
  const int64_t n = t.info.total_samples;
  const int64_t i0 = ((int64_t)blockIdx.x * MIX_THREADS + threadIdx.x) * BT_FLAC_THREAD_SAMPLES;
  if (i0 >= n) return;
  const Layout l = layout(t.info);
  const int32_t* pl = (const int32_t*)t.ws + i0;   // (ld is a multiple of 4 and the workspace 16-byte aligned: aligned 16-byte loads)
  float v[4];
  mix4([&](int c) {
    const i32x4 q = *(const i32x4*)(pl + (int64_t)c * l.ld);
    return Quad{{q.x, q.y, q.z, q.w}};
  }, t.info.channels, 1.0 / (double)(1u << (t.info.bps - 1)), v);
  float* o = t.out + i0;
  if (n - i0 >= BT_FLAC_THREAD_SAMPLES) {
    *(f32x4*)o = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < BT_FLAC_THREAD_SAMPLES - 1; ++j)
      if (j < n - i0) o[j] = v[j];
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
int fail(const char* fn, const char* msg, int code = BT_ERR_ARG) {
  return bt_set_error_external(code, (std::string(fn) + ": " + msg).c_str());
}

// null: fine; else what is wrong with the span
const char* span_problem(const Span& s) {
  if (!s.src || !s.out || !s.ws || !s.status) return "null pointer in a span";
  if (!info_ok(s.info, true)) return "a bt_flac_info outside the decoder's subset (or 2^31 bytes / samples or more)";
  if (((uintptr_t)s.out & 15) || ((uintptr_t)s.ws & 15)) return "d_out and d_ws must be 16-byte aligned";
  return nullptr;
}

int launch(const char* fn, hipStream_t st, const Span& one, const Span* d_tracks, int n_tracks, int64_t max_nblk, int64_t max_cap,
           int64_t max_samples) {
  const dim3 scan((unsigned)max_nblk, (unsigned)n_tracks), per_track(1, (unsigned)n_tracks);
  const dim3 walk((unsigned)((max_cap + WALK - 1) / WALK), (unsigned)n_tracks);
  const dim3 mix((unsigned)((max_samples + BT_FLAC_BLOCK_SAMPLES - 1) / BT_FLAC_BLOCK_SAMPLES), (unsigned)n_tracks);
  hipLaunchKernelGGL(flac_scan_kernel, scan, dim3(SCAN), 0, st, one, d_tracks);
  hipLaunchKernelGGL(flac_prefix_kernel, per_track, dim3(256), 0, st, one, d_tracks);
  hipLaunchKernelGGL(flac_compact_kernel, scan, dim3(SCAN), 0, st, one, d_tracks);
  hipLaunchKernelGGL(flac_measure_kernel, walk, dim3(WALK), 0, st, one, d_tracks);
  hipLaunchKernelGGL(flac_link_kernel, per_track, dim3(64), 0, st, one, d_tracks);
  hipLaunchKernelGGL(flac_decode_kernel, walk, dim3(WALK), 0, st, one, d_tracks);
  hipLaunchKernelGGL(flac_mix_kernel, mix, dim3(MIX_THREADS), 0, st, one, d_tracks);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? BT_OK : fail(fn, hipGetErrorString(e), BT_ERR_HIP);
}

}  // namespace

extern "C" {

int bt_flac_probe_host(const uint8_t* bytes, int64_t n_bytes, bt_flac_info* info) {
  return flac::probe(bytes, n_bytes, reinterpret_cast<Info*>(info));
}

size_t bt_flac_workspace_bytes(const bt_flac_info* info) {
  if (!info || !info_ok(*reinterpret_cast<const Info*>(info), true)) return 0;
  return layout(*reinterpret_cast<const Info*>(info)).total;
}

int bt_flac_decode_host(const uint8_t* src, const bt_flac_info* info, float* out_f32, int32_t* pcm_i32_or_null, bt_flac_status* status) {
  const char* fn = "bt_flac_decode_host";
  if (!src || !info || !out_f32 || !status) return fail(fn, "null argument");
  const Info& in = *reinterpret_cast<const Info*>(info);
  if (!info_ok(in, false)) return fail(fn, "a bt_flac_info outside the decoder's subset");
  const int64_t ld = (in.total_samples + 3) / 4 * 4;
  std::vector<int32_t> planar((size_t)in.channels * (size_t)ld, 0);
  flac::Status st;
  flac::decode_chain_host(src, in, planar.data(), ld, &st);
  memcpy(status, &st, sizeof st);
  if (st.code != FL_OK) return BT_OK;
  const double scale = 1.0 / (double)(1u << (in.bps - 1));
  for (int64_t i0 = 0; i0 < in.total_samples; i0 += 4) {
    float v[4];
    mix4([&](int c) {
      Quad q;
      memcpy(q.v, planar.data() + (size_t)c * ld + i0, 16);
      return q;
    }, in.channels, scale, v);
    for (int j = 0; j < 4 && i0 + j < in.total_samples; ++j) out_f32[i0 + j] = v[j];
  }
  if (pcm_i32_or_null)
    for (int64_t i = 0; i < in.total_samples; ++i)
      for (int c = 0; c < in.channels; ++c) pcm_i32_or_null[i * in.channels + c] = planar[(size_t)c * ld + i];
  return BT_OK;
}

int bt_flac_decode_batch(void* stream, const bt_flac_span* h_tracks, const bt_flac_span* d_tracks, int n_tracks) {
  const char* fn = "bt_flac_decode_batch";
  if (!h_tracks || !d_tracks) return fail(fn, "null argument");
  if (n_tracks < 0) return fail(fn, "negative count");
  if (n_tracks > BT_FLAC_MAX_TRACKS) return fail(fn, "more than BT_FLAC_MAX_TRACKS tracks");
  if (n_tracks == 0) return BT_OK;
  int64_t max_nblk = 0, max_cap = 0, max_samples = 0;
  for (int k = 0; k < n_tracks; ++k) {
    const Span& s = reinterpret_cast<const Span*>(h_tracks)[k];
    if (const char* msg = span_problem(s)) return fail(fn, msg);
    const Layout l = layout(s.info);
    if (s.ws_bytes < l.total) return fail(fn, "a track's workspace is smaller than bt_flac_workspace_bytes", BT_ERR_WORKSPACE);
    max_nblk = l.nblk > max_nblk ? l.nblk : max_nblk;
    max_cap = l.cap > max_cap ? l.cap : max_cap;
    max_samples = s.info.total_samples > max_samples ? s.info.total_samples : max_samples;
  }
  return launch(fn, (hipStream_t)stream, Span{}, reinterpret_cast<const Span*>(d_tracks), n_tracks, max_nblk, max_cap, max_samples);
}

int bt_flac_decode(void* stream, const uint8_t* d_src, const bt_flac_info* info, float* d_out, void* d_ws, size_t ws_bytes,
                   bt_flac_status* d_status) {
  const char* fn = "bt_flac_decode";
  if (!info) return fail(fn, "null argument");
  Span s{d_src, d_out, d_ws, ws_bytes, reinterpret_cast<flac::Status*>(d_status), *reinterpret_cast<const Info*>(info)};
  if (const char* msg = span_problem(s)) return fail(fn, msg);
  const Layout l = layout(s.info);
  if (ws_bytes < l.total) return fail(fn, "the workspace is smaller than bt_flac_workspace_bytes", BT_ERR_WORKSPACE);
  return launch(fn, (hipStream_t)stream, s, nullptr, 1, l.nblk, l.cap, s.info.total_samples);
}

}  // extern "C"
