// Training batches: what the reference's BeatTrackingDataset.__getitem__ (beat_this/dataset/dataset.py) and torch's collate
// produce for a batch of items, from a spectrogram store that stays in device memory.  DESIGN.md section 12.
//
// The host plans a batch (which excerpt of which piece, which mask operations, drawn from np.random exactly as the reference
// draws them) into three small tables; the frames themselves are never touched by the host.  One launch: workgroup
// (item b, block of FB frames) resolves, for each of its output frames, the store row it shows -- the reference applies its mask
// operations one after the other IN PLACE, so the frame at t after the last operation is found by walking the operations
// from the last to the first and mapping t back through every permutation that covers it -- and copies that row (or zeros)
// with 16-byte accesses, 16 lanes per row.  The same workgroup writes the framewise targets of its frames in gather form:
// it finds the first annotation whose frame reaches the block by bisection, raises flags in LDS for the annotations inside
// the block and stores them coalesced.  Every output byte is written by exactly one thread: no memset, no atomics.
// Host: bt_train_batch_host runs the same resolve / frame functions (they are __host__ __device__, integer and fp64 only;
// the file is compiled with -ffp-contract=off) and the same conversions: its outputs are bit-identical.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/beat_this_amd.h"

#pragma clang fp contract(off)

int bt_set_error_external(int code, const char* msg);   // engine.hip (bt_last_error)

namespace {

constexpr int FB = BT_TRAIN_FRAME_BLOCK;   // frames per workgroup
constexpr int THREADS = 256;               // 16 rows of 16 lanes per pass
constexpr int W = 128;                     // spectrogram bins

struct Tables {
  const bt_train_op* ops;
  const bt_train_part* parts;
  const double* ann_time;
  const int32_t* ann_value;
  int n_ops, n_parts;
  int64_t n_ann;
  double fps;
};

// ---- exact conversions, the same integer operations on host and device -------------------------------------------------------
__host__ __device__ inline uint32_t h2f_bits(uint32_t h) {   // fp16 bits -> fp32 bits
  const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 0x1f, m = h & 0x3ff;
  if (e == 0) {
    if (m == 0) return s;
    int k = 0;   // subnormal m * 2^-24: normalise
    uint32_t mm = m;
    while (!(mm & 0x400)) {
      mm <<= 1;
      ++k;
    }
    return s | ((uint32_t)(113 - k) << 23) | ((mm & 0x3ff) << 13);
  }
  if (e == 31) return s | 0x7f800000u | (m << 13);
  return s | ((e + 112) << 23) | (m << 13);
}

__host__ __device__ inline uint32_t f2h_bits(uint32_t x) {   // fp32 bits -> fp16 bits, round to nearest even
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return sign | 0x7c00u | (x > 0x7f800000u ? (0x200u | ((x >> 13) & 0x3ffu)) : 0u);
  if (x >= 0x477ff000u) return sign | 0x7c00u;   // 65520 and above round to infinity
  if (x < 0x38800000u) {                         // below 2^-14: a subnormal half (units of 2^-24) or zero
    if (x < 0x33000000u) return sign;            // below 2^-25
    const int shift = 126 - (int)(x >> 23);      // 14 .. 24
    const uint32_t m = (x & 0x7fffffu) | 0x800000u, half = 1u << (shift - 1), rem = m & ((1u << shift) - 1);
    uint32_t r = m >> shift;
    if (rem > half || (rem == half && (r & 1))) ++r;
    return sign | r;
  }
  uint32_t r = (x - 0x38000000u) >> 13;
  const uint32_t rem = x & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (r & 1))) ++r;
  return sign | r;
}

// ---- the plan, read the same way on host and device ---------------------------------------------------------------------------
// Excerpt frame shown at output frame t (0 <= t < n) after the item's mask operations, or -1: a zeroed frame.  Entries that
// point outside their tables give -1 (the host twin refuses them beforehand).
__host__ __device__ inline int resolve_frame(const Tables& tb, int op_begin, int op_end, int t, int n) {
  if (op_begin < 0 || op_end > tb.n_ops) return op_begin < op_end ? -1 : t;
  for (int k = op_end - 1; k >= op_begin; --k) {
    const bt_train_op op = tb.ops[k];
    const int64_t u = (int64_t)t - op.start;
    if (u < 0 || u >= op.length) continue;
    if (op.kind != BT_MASK_PERMUTE) return -1;
    int lo = op.part_begin, hi = op.part_end;
    if (lo < 0 || hi > tb.n_parts || lo >= hi) return -1;
    while (hi - lo > 1) {   // the last part whose new_off <= u
      const int mid = lo + (hi - lo) / 2;
      if (tb.parts[mid].new_off <= u) lo = mid;
      else hi = mid;
    }
    const bt_train_part p = tb.parts[lo];
    const int64_t t2 = (int64_t)op.start + p.old_off + (u - p.new_off);
    if (t2 < 0 || t2 >= n) return -1;
    t = (int)t2;
  }
  return t;
}

// frame of an annotation relative to the excerpt: np.round(time * fps) - start_frame, in fp64
__host__ __device__ inline double ann_frame(double time, double fps, int start_frame) {
  return rint(time * fps) - (double)start_frame;
}

// first annotation in [lo, hi) whose frame is >= t0 (frames ascend with the times)
__host__ __device__ inline int64_t first_annotation(const Tables& tb, int64_t lo, int64_t hi, int start_frame, double t0) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (ann_frame(tb.ann_time[mid], tb.fps, start_frame) >= t0) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

struct DevArgs {
  Tables tb;
  const void* store;
  const bt_train_item* items;
  void* spect;
  uint8_t *truth_beat, *truth_downbeat, *padding_mask, *downbeat_mask;
  int64_t store_rows;
  int store_dtype, spect_dtype, L, nblk;
};

__device__ inline uint4 halves_of(const uint4 a, const uint4 b) {   // 8 floats (bits) -> 8 halves
  uint4 r;
  r.x = f2h_bits(a.x) | (f2h_bits(a.y) << 16);
  r.y = f2h_bits(a.z) | (f2h_bits(a.w) << 16);
  r.z = f2h_bits(b.x) | (f2h_bits(b.y) << 16);
  r.w = f2h_bits(b.z) | (f2h_bits(b.w) << 16);
  return r;
}

__global__ __launch_bounds__(THREADS) void train_batch_kernel(const DevArgs a) {
  __shared__ int64_t s_row[FB];            // store row of each frame of the block, -1: zeros
  __shared__ uint8_t s_beat[FB], s_down[FB];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.nblk, t0 = (blockIdx.x % a.nblk) * FB;
  const bt_train_item it = a.items[b];
  const int n = it.n < 0 ? 0 : (it.n > a.L ? a.L : it.n);
  if (tid < FB) {
    const int t = t0 + tid;
    int64_t row = -1;
    if (t < n) {
      const int src = resolve_frame(a.tb, it.op_begin, it.op_end, t, n);
      if (src >= 0) {
        row = it.row + src;
        if (row < 0 || row >= a.store_rows) row = -1;
      }
    }
    s_row[tid] = row;
    s_beat[tid] = 0;
    s_down[tid] = 0;
  }
  __syncthreads();
  if (a.truth_beat || a.truth_downbeat) {
    const int t1 = t0 + FB < n ? t0 + FB : n;   // annotations count on frames [t0, t1)
    int64_t lo = it.ann_begin < 0 ? 0 : it.ann_begin, hi = it.ann_end > a.tb.n_ann ? a.tb.n_ann : it.ann_end;
    if (t0 < t1 && lo < hi) {
      const int64_t first = first_annotation(a.tb, lo, hi, it.start_frame, (double)t0);
      for (int64_t i = first + tid; i < hi; i += THREADS) {
        const double f = ann_frame(a.tb.ann_time[i], a.tb.fps, it.start_frame);
        if (!(f < (double)t1)) break;
        if (f >= (double)t0) {
          const int j = (int)f - t0;
          s_beat[j] = 1;
          if (a.tb.ann_value[i] == 1) s_down[j] = 1;
        }
      }
    }
  }
  __syncthreads();
  if (tid < FB && t0 + tid < a.L) {
    const int64_t o = (int64_t)b * a.L + t0 + tid;
    if (a.truth_beat) a.truth_beat[o] = s_beat[tid];
    if (a.truth_downbeat) a.truth_downbeat[o] = s_down[tid];
    if (a.padding_mask) a.padding_mask[o] = t0 + tid < n ? 1 : 0;
  }
  if (a.downbeat_mask && t0 == 0 && tid == 0) a.downbeat_mask[b] = it.has_downbeats != 0 ? 1 : 0;
  if (!a.spect) return;
  const int lane = tid & 15;
  for (int r = tid >> 4; r < FB && t0 + r < a.L; r += THREADS / 16) {
    const int64_t row = s_row[r];
    const int64_t o = ((int64_t)b * a.L + t0 + r) * W;   // first element of the output row
    uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0;
    if (a.store_dtype == BT_LOSS_F16) {
      if (row >= 0) v0 = ((const uint4*)a.store)[row * (W / 8) + lane];   // 8 halves
      if (a.spect_dtype == BT_LOSS_F16) {
        ((uint4*)a.spect)[o / 8 + lane] = v0;
      } else {
        uint4* out = (uint4*)a.spect + o / 4 + 2 * lane;
        out[0] = make_uint4(h2f_bits(v0.x & 0xffff), h2f_bits(v0.x >> 16), h2f_bits(v0.y & 0xffff), h2f_bits(v0.y >> 16));
        out[1] = make_uint4(h2f_bits(v0.z & 0xffff), h2f_bits(v0.z >> 16), h2f_bits(v0.w & 0xffff), h2f_bits(v0.w >> 16));
      }
    } else if (a.spect_dtype == BT_LOSS_F32) {   // floats [4 lane, +4) and [64 + 4 lane, +4): contiguous over the lanes
      if (row >= 0) {
        const uint4* in = (const uint4*)a.store + row * (W / 4);
        v0 = in[lane];
        v1 = in[16 + lane];
      }
      uint4* out = (uint4*)a.spect + o / 4;
      out[lane] = v0;
      out[16 + lane] = v1;
    } else {
      if (row >= 0) {
        const uint4* in = (const uint4*)a.store + row * (W / 4) + 2 * lane;   // 8 floats
        v0 = in[0];
        v1 = in[1];
      }
      ((uint4*)a.spect)[o / 8 + lane] = halves_of(v0, v1);
    }
  }
}

int fail(const char* who, const std::string& msg) { return bt_set_error_external(BT_ERR_ARG, (std::string(who) + ": " + msg).c_str()); }

bool common_args_bad(const void* store, int store_dtype, int64_t store_rows, const void* items, int B, int L, const void* ops,
                     int n_ops, const void* parts, int n_parts, const void* ann_time, const void* ann_value, int64_t n_ann,
                     double fps, const void* spect, int spect_dtype) {
  return !items || B <= 0 || L <= 0 || store_rows < 0 || (store_rows > 0 && !store) || n_ops < 0 || (n_ops > 0 && !ops) ||
         n_parts < 0 || (n_parts > 0 && !parts) || n_ann < 0 || (n_ann > 0 && (!ann_time || !ann_value)) || !(fps > 0.0) ||
         (store_dtype != BT_LOSS_F16 && store_dtype != BT_LOSS_F32) ||
         (spect && spect_dtype != BT_LOSS_F16 && spect_dtype != BT_LOSS_F32);
}

}  // namespace

void bt_train_batch_struct_sizes(int32_t* out) {
  out[0] = (int32_t)sizeof(bt_train_item);
  out[1] = (int32_t)sizeof(bt_train_op);
  out[2] = (int32_t)sizeof(bt_train_part);
  out[3] = (int32_t)offsetof(bt_train_item, ann_begin);
  out[4] = (int32_t)offsetof(bt_train_item, n);
  out[5] = (int32_t)offsetof(bt_train_item, op_begin);
  out[6] = (int32_t)offsetof(bt_train_item, has_downbeats);
  out[7] = (int32_t)offsetof(bt_train_op, kind);
  out[8] = (int32_t)offsetof(bt_train_op, part_begin);
  out[9] = (int32_t)offsetof(bt_train_part, old_off);
}

int bt_train_batch(void* stream, const void* d_store, int store_dtype, int64_t store_rows, const bt_train_item* d_items, int B,
                   int L, const bt_train_op* d_ops, int n_ops, const bt_train_part* d_parts, int n_parts,
                   const double* d_ann_time, const int32_t* d_ann_value, int64_t n_ann, double fps, void* d_spect,
                   int spect_dtype, uint8_t* d_truth_beat, uint8_t* d_truth_downbeat, uint8_t* d_padding_mask,
                   uint8_t* d_downbeat_mask) {
  if (common_args_bad(d_store, store_dtype, store_rows, d_items, B, L, d_ops, n_ops, d_parts, n_parts, d_ann_time, d_ann_value,
                      n_ann, fps, d_spect, spect_dtype))
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_train_batch");
  if (((uintptr_t)d_store | (uintptr_t)d_spect) & 15)
    return bt_set_error_external(BT_ERR_ARG, "bt_train_batch: the store and the spectrogram output must be 16-byte aligned");
  const int64_t nblk = ((int64_t)L + FB - 1) / FB;
  if (nblk * B > 0x7fffffff) return bt_set_error_external(BT_ERR_ARG, "bt_train_batch: too many frame blocks");
  DevArgs a{};
  a.tb = Tables{d_ops, d_parts, d_ann_time, d_ann_value, n_ops, n_parts, n_ann, fps};
  a.store = d_store;
  a.items = d_items;
  a.spect = d_spect;
  a.truth_beat = d_truth_beat;
  a.truth_downbeat = d_truth_downbeat;
  a.padding_mask = d_padding_mask;
  a.downbeat_mask = d_downbeat_mask;
  a.store_rows = store_rows;
  a.store_dtype = store_dtype;
  a.spect_dtype = spect_dtype;
  a.L = L;
  a.nblk = (int)nblk;
  hipLaunchKernelGGL(train_batch_kernel, dim3((unsigned)(nblk * B)), dim3(THREADS), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return bt_set_error_external(BT_ERR_HIP, (std::string("bt_train_batch: ") + hipGetErrorString(e)).c_str());
  return BT_OK;
}

int bt_train_batch_host(const void* store, int store_dtype, int64_t store_rows, const bt_train_item* items, int B, int L,
                        const bt_train_op* ops, int n_ops, const bt_train_part* parts, int n_parts, const double* ann_time,
                        const int32_t* ann_value, int64_t n_ann, double fps, void* spect, int spect_dtype, uint8_t* truth_beat,
                        uint8_t* truth_downbeat, uint8_t* padding_mask, uint8_t* downbeat_mask) {
  const char* who = "bt_train_batch_host";
  if (common_args_bad(store, store_dtype, store_rows, items, B, L, ops, n_ops, parts, n_parts, ann_time, ann_value, n_ann, fps,
                      spect, spect_dtype))
    return bt_set_error_external(BT_ERR_ARG, "bad argument to bt_train_batch_host");
  for (int b = 0; b < B; ++b) {
    const bt_train_item& it = items[b];
    const std::string name = "item " + std::to_string(b);
    if (it.n < 0 || it.n > L) return fail(who, name + " has " + std::to_string(it.n) + " frames, the batch " + std::to_string(L));
    if (it.row < 0 || it.row > store_rows - it.n) return fail(who, name + " reaches outside the store");
    if (it.op_begin < 0 || it.op_end < it.op_begin || it.op_end > n_ops) return fail(who, name + ": op range outside the table");
    if (it.ann_begin < 0 || it.ann_end < it.ann_begin || it.ann_end > n_ann)
      return fail(who, name + ": annotation range outside the arrays");
    for (int k = it.op_begin; k < it.op_end; ++k) {
      const bt_train_op& op = ops[k];
      const std::string oname = name + ", op " + std::to_string(k);
      if (op.start < 0 || op.length < 0 || (int64_t)op.start + op.length > it.n) return fail(who, oname + " reaches outside the excerpt");
      if (op.kind != BT_MASK_ZERO && op.kind != BT_MASK_PERMUTE) return fail(who, oname + ": unknown kind");
      if (op.kind != BT_MASK_PERMUTE || op.length == 0) continue;
      if (op.part_begin < 0 || op.part_end <= op.part_begin || op.part_end > n_parts) return fail(who, oname + ": part range outside the table");
      for (int p = op.part_begin; p < op.part_end; ++p) {
        const int32_t begin = parts[p].new_off, end = p + 1 < op.part_end ? parts[p + 1].new_off : op.length;
        if ((p == op.part_begin && begin != 0) || end <= begin || end > op.length || parts[p].old_off < 0 ||
            (int64_t)parts[p].old_off + (end - begin) > op.length)
          return fail(who, oname + ", part " + std::to_string(p) + ": not an ascending split of the op's frames");
      }
    }
  }
  const Tables tb{ops, parts, ann_time, ann_value, n_ops, n_parts, n_ann, fps};
  const size_t in_elt = store_dtype == BT_LOSS_F16 ? 2 : 4, out_elt = spect_dtype == BT_LOSS_F16 ? 2 : 4;
  for (int b = 0; b < B; ++b) {
    const bt_train_item& it = items[b];
    const int n = it.n;
    if (downbeat_mask) downbeat_mask[b] = it.has_downbeats != 0 ? 1 : 0;
    for (int t = 0; t < L; ++t) {
      const int64_t o = (int64_t)b * L + t;
      if (truth_beat) truth_beat[o] = 0;
      if (truth_downbeat) truth_downbeat[o] = 0;
      if (padding_mask) padding_mask[o] = t < n ? 1 : 0;
      if (!spect) continue;
      char* out = (char*)spect + (size_t)o * W * out_elt;
      const int src = t < n ? resolve_frame(tb, it.op_begin, it.op_end, t, n) : -1;
      if (src < 0) {
        memset(out, 0, W * out_elt);
        continue;
      }
      const char* in = (const char*)store + (size_t)(it.row + src) * W * in_elt;
      if (in_elt == out_elt) {
        memcpy(out, in, W * in_elt);
      } else if (in_elt == 2) {
        for (int c = 0; c < W; ++c) {
          uint16_t h;
          memcpy(&h, in + 2 * c, 2);
          const uint32_t f = h2f_bits(h);
          memcpy(out + 4 * c, &f, 4);
        }
      } else {
        for (int c = 0; c < W; ++c) {
          uint32_t f;
          memcpy(&f, in + 4 * c, 4);
          const uint16_t h = (uint16_t)f2h_bits(f);
          memcpy(out + 2 * c, &h, 2);
        }
      }
    }
    if (truth_beat || truth_downbeat) {
      const int64_t first = first_annotation(tb, it.ann_begin, it.ann_end, it.start_frame, 0.0);
      for (int64_t i = first; i < it.ann_end; ++i) {
        const double f = ann_frame(ann_time[i], fps, it.start_frame);
        if (!(f < (double)n)) break;
        if (f >= 0.0) {
          const int64_t o = (int64_t)b * L + (int)f;
          if (truth_beat) truth_beat[o] = 1;
          if (truth_downbeat && ann_value[i] == 1) truth_downbeat[o] = 1;
        }
      }
    }
  }
  return BT_OK;
}
