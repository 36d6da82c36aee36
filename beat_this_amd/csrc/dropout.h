// Dropout masks of the training route: Philox4x32-10, a counter-based generator that the kernels
// evaluate where they need a mask bit and that the host evaluates the same way (bt_dropout_mask_host), so no mask is ever
// stored.  The contract -- which counter and which of its four words belong to an element -- is written out in
// include/beat_this_amd.h; this file is its only implementation, for the device and the host alike.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define BT_DROP_FN __host__ __device__ inline
#else
#define BT_DROP_FN inline
#endif

struct PhiloxWords {
  uint32_t w[4];
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011; the constants of Random123)
BT_DROP_FN PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return PhiloxWords{{c0, c1, c2, c3}};
}

// One site of one unit call, passed to the kernels by value.  Counter of element group g (64-bit):
//   { g mod 2^32,  site << 24 | g >> 32,  stream mod 2^32,  stream >> 32 },  key = { seed mod 2^32, seed >> 32 }
struct DropSite {
  uint32_t thr;      // keep iff word >= thr;  thr = floor(p 2^32)
  float scale;       // 1 / (1 - p), what a kept value is multiplied by
  uint32_t key0, key1, site, stream0, stream1;
};

BT_DROP_FN DropSite drop_site(float p, uint64_t seed, uint64_t stream, int site) {
  DropSite s;
  s.thr = (uint32_t)((double)p * 4294967296.0);   // (0 <= p < 1: the product is below 2^32; the conversion truncates)
  s.scale = 1.0f / (1.0f - p);
  s.key0 = (uint32_t)seed;
  s.key1 = (uint32_t)(seed >> 32);
  s.site = (uint32_t)site << 24;
  s.stream0 = (uint32_t)stream;
  s.stream1 = (uint32_t)(stream >> 32);
  return s;
}

BT_DROP_FN PhiloxWords drop_words(const DropSite& s, uint64_t group) {
  return philox4x32_10((uint32_t)group, s.site | (uint32_t)(group >> 32), s.stream0, s.stream1, s.key0, s.key1);
}

// Element -> (group, word).  Row sites [rows][n], n a multiple of 4: four consecutive columns of one row share a call.
BT_DROP_FN uint64_t drop_row_group(uint64_t row, uint32_t n, uint32_t col) { return row * (n >> 2) + (col >> 2); }
// The attention probabilities [B][H][T][T]: four consecutive keys of one query share a call; a query has (T + 3) / 4 groups,
// and the words of the last one that lie behind key T - 1 are not used.
BT_DROP_FN uint64_t drop_attn_group(uint64_t bh, uint32_t T, uint32_t q, uint32_t k) {
  return (bh * T + q) * ((T + 3) >> 2) + (k >> 2);
}
