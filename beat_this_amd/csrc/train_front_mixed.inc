// The 16-mixed conv unit of the differentiable frontend (DESIGN.md section 19), included by train_front.hip inside its
// namespace, behind ConvP, ConvTile<MODE> and conv_store<MODE>: the three products of the fp32 conv_gemm_kernel in its frame and
// with its epilogue; the staging and the MFMA loop are this file's own.
// THE CONTRACT is section 16's: both operands of pre = A W^T, g_x = G W and g_W = G^T A are rounded to IEEE fp16 (to nearest
// even, beyond its range: inf) as they are staged, G = g_pre s being multiplied in fp32 first, and the products accumulate in
// fp32 on v_mfma_f32_32x32x16_f16.  Nothing clamps.  Everything around the products is the fp32 code of train_front.hip.
// The kernels are templates over the operand element type E (Operand<E>, train_common.h): _Float16 is the above, __bf16 (section
// 24) rounds to bfloat16 instead -- NaN stays NaN, nothing overflows -- on v_mfma_f32_32x32x16_bf16, the weight image in the
// same bytes.  bf16x3 (section 25) keeps two bfloat16 images of every operand, hi and lo (to_img, train_common.h): the packed
// weight is a hi image followed by a lo image, the staged tiles are pairs, and a k-step issues lo hi, hi lo, hi hi.
//
// Lane maps of the 32x32x16 fp16 MFMA (train_mixed.inc): lane l, r = l & 31, h = l >> 5, element j = 0 .. 7 of a fragment is
// A[row r][k = 8 h + j] and B[k = 8 h + j][col r]; C / D register i is row (i & 3) + 8 (i >> 2) + 4 h, col r.  Both operand tiles
// lie in LDS as [row or col][k] with MLD = MK + 8 halves per row, so a fragment is one 16-byte read and the reads of 32 rows
// spread over the banks.
//
// Staging.  A row of the implicit A (MODE 0) is three contiguous runs of 2 Cin floats (frames t - 1, t, t + 1), a row of G
// (MODE 1) three runs of Cout floats (frames t + 1, t, t - 1); both run lengths are multiples of 64, so a k-step of MK = 32
// lies inside one run: the frame of a row is computed once per row, the boundary test and the address once per row and
// k-step, and the loads are 16 bytes wide.  MODE 2 sums over the rows: its tiles are read along the columns (64 columns of one
// run, again 16-byte loads) and written to LDS transposed.  The weight w[co][ci][df][dt] has dt fastest; a launch at the head of
// the call packs it once into an fp16 image in the workspace, [co][dt 2 Cin + df Cin + ci] for MODE 0 and
// [df Cin + ci][dt Cout + co] for MODE 1 -- the same values rounded the same way, read back with 16-byte loads.
// The next k-step's global loads are issued before the current step's MFMAs.
//
// Orders of summation (functions of the shapes alone): a forward or backward-data element sums k ascending in MFMA steps of 16;
// g_W sums the rows ascending in steps of 16 inside each chunk of BT_TRAIN_DW_ROWS rows, and conv_dw_reduce_kernel adds the
// chunks in order.  No atomics, one thread of one launch per output byte, a row's results depend on its own sequence only.

constexpr int MK = 32;         // k per staging step: two MFMA steps
constexpr int MLD = MK + 8;    // halves per LDS row (80 bytes)

__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
__device__ inline f32x4 load4(const float* p, bool vec) {
  return vec ? *reinterpret_cast<const f32x4*>(p) : f32x4{p[0], p[1], p[2], p[3]};
}

// img [Cout][6 Cin] (transposed == 0: k = dt 2 Cin + df Cin + ci) or [2 Cin][3 Cout] (k = dt Cout + co) = E(w[co][ci][df][dt])
// (bf16x3: the lo image follows the hi image, Cout 6 Cin elements further)
template <typename E>
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* w, int Cout, int Cin, int transposed, el16<E>* img) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Cout * 6 * Cin) return;
  int co, j, dt;
  if (!transposed) {
    const int k = i % (6 * Cin);
    co = i / (6 * Cin);
    dt = k / (2 * Cin);
    j = k - dt * 2 * Cin;
  } else {
    const int k = i % (3 * Cout);
    j = i / (3 * Cout);
    dt = k / Cout;
    co = k - dt * Cout;
  }
  const int df = j / Cin, ci = j - df * Cin;
  el16<E> e[Operand<E>::NI];
  to_img<E>(w[((long)co * Cin + ci) * 6 + df * 3 + dt], e);
#pragma unroll
  for (int n = 0; n < Operand<E>::NI; ++n) img[(long)n * Cout * 6 * Cin + i] = e[n];
}

// conv_gemm_kernel<MODE> with operands of type E: the same grid, tile and epilogue.  p.wh: the packed weight (MODE 0 and 1).
template <typename E, int MODE>
__global__ __launch_bounds__(256) void conv_gemm_mixed_kernel(const ConvP p) {
  constexpr int NI = Operand<E>::NI;
  __shared__ __attribute__((aligned(16))) el16<E> As[NI][GT][MLD];
  __shared__ __attribute__((aligned(16))) el16<E> Bs[NI][GT][MLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 5, lr = lane & 31, wm = wave >> 1, wn = wave & 1;
  const ConvTile<MODE> tile(p);
  const bool vx = aligned16(p.x), vg = aligned16(p.g);
  const int run = MODE == 1 ? p.Cout : tile.C2;   // floats per frame of a row of the staged activation
  const int KW = 3 * run;                    // MODE 0 / 1: halves per row of the weight image

  // MODE 0 / 1: this thread stages four k of rows (tid >> 3) and 32 + (tid >> 3) of A and eight k of row tid >> 2 of the image
  // MODE 2: four columns 4 (tid & 15) of the summed rows (tid >> 4) and 16 + (tid >> 4), of both operands
  int row_t[2] = {-4, -4};   // the frame of the thread's two rows (MODE 0 / 1); -4: no such row
  if (MODE != 2) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const long gm = tile.m0 + i * 32 + (tid >> 3);
      if (gm < tile.GM) row_t[i] = (int)((gm / p.Fo) % p.T);
    }
  }
  const int dt2 = tile.n0 / tile.C2, j2 = tile.n0 - dt2 * tile.C2;   // MODE 2: the run and the first column of this tile of the implicit A

  Img4<E> ra[2], rb[2];
  Img8<E> rw;
  auto fetch = [&](long k0) {
    if constexpr (MODE != 2) {
      const int dt = (int)(k0 / run), j0 = (int)(k0 - (long)dt * run);
      const int sh = MODE == 0 ? dt - 1 : 1 - dt;   // the source row lies sh frames from the output row
      const int kk = (tid & 7) * 4;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const long gm = tile.m0 + i * 32 + (tid >> 3);
        const int t = row_t[i] + sh;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row_t[i] >= 0 && t >= 0 && t < p.T) {
          v = load4((MODE == 0 ? p.x : p.g) + (gm + (long)sh * p.Fo) * run + j0 + kk, MODE == 0 ? vx : vg);
          if (MODE == 1) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] *= p.fold[j0 + kk + c];
          }
        }
        ra[i] = to_h4<E>(v);
      }
      const int gn = tile.n0 + (tid >> 2);
#pragma unroll
      for (int n = 0; n < NI; ++n) {
        rw.v[n] = h16x8<E>{0, 0, 0, 0, 0, 0, 0, 0};
        if (gn < tile.GN)
          rw.v[n] = *reinterpret_cast<const h16x8<E>*>((const el16<E>*)p.wh + (long)n * p.Cout * 6 * p.Cin + (long)gn * KW + k0 + (tid & 3) * 8);
      }
    } else {
      const int c4 = (tid & 15) * 4;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const long gk = k0 + i * 16 + (tid >> 4);
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (gk < tile.ke) {
          if (tile.m0 + c4 < tile.GM) {
            a = load4(p.g + gk * p.Cout + tile.m0 + c4, vg);
#pragma unroll
            for (int c = 0; c < 4; ++c) a[c] *= p.fold[tile.m0 + c4 + c];
          }
          const int t = (int)((gk / p.Fo) % p.T) + dt2 - 1;
          if (tile.n0 + c4 < tile.GN && t >= 0 && t < p.T) b = load4(p.x + (gk + (long)(dt2 - 1) * p.Fo) * tile.C2 + j2 + c4, vx);
        }
        ra[i] = to_h4<E>(a);
        rb[i] = to_h4<E>(b);
      }
    }
  };
  auto commit = [&]() {
    if constexpr (MODE != 2) {
#pragma unroll
      for (int n = 0; n < NI; ++n) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<h16x4<E>*>(&As[n][i * 32 + (tid >> 3)][(tid & 7) * 4]) = ra[i].v[n];
        *reinterpret_cast<h16x8<E>*>(&Bs[n][tid >> 2][(tid & 3) * 8]) = rw.v[n];
      }
    } else {
      const int c4 = (tid & 15) * 4;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int kk = i * 16 + (tid >> 4);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int n = 0; n < NI; ++n) {
            As[n][c4 + c][kk] = ra[i].v[n][c];
            Bs[n][c4 + c][kk] = rb[i].v[n][c];
          }
      }
    }
  };

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  fetch(tile.kb);
  for (long k0 = tile.kb; k0 < tile.ke; k0 += MK) {
    commit();
    __syncthreads();
    if (k0 + MK < tile.ke) fetch(k0 + MK);
#pragma unroll
    for (int s = 0; s < MK / 16; ++s) {
      Img8<E> a, b;
#pragma unroll
      for (int n = 0; n < NI; ++n) {
        a.v[n] = *reinterpret_cast<const h16x8<E>*>(&As[n][wm * 32 + lr][16 * s + 8 * g]);
        b.v[n] = *reinterpret_cast<const h16x8<E>*>(&Bs[n][wn * 32 + lr][16 * s + 8 * g]);
      }
      acc = mfma_terms<E>(a, b, acc);
    }
    __syncthreads();
  }
  conv_store<MODE>(p, tile, acc, wm, wn, lr, g);
}
