/* beat_this_amd -- C ABI of the MI355X-native beat_this inference hot path.
 *
 * The reference (CPJKU/beat_this, pure Python) has no FFI; its seam is the Python
 * API of beat_this/inference.py.  These entry points are what a binding for that
 * seam calls -- each one cites the reference code it replaces.  All `d_*` pointers
 * are DEVICE pointers owned by the caller (torch tensors on the Python side);
 * `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream).  No call
 * allocates device memory, synchronises the device, or starts threads.  Return
 * value: BT_OK or a negative BT_ERR_* code; bt_last_error() gives the text.
 * The library is reentrant per engine handle, not concurrently on one handle; the caller's workspace belongs to ONE
 * stream at a time (two streams running one engine need two workspaces).
 */
#ifndef BEAT_THIS_AMD_H
#define BEAT_THIS_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_OK 0
#define BT_ERR_ARG (-1)      /* bad argument / unsupported shape  -> ValueError */
#define BT_ERR_HIP (-2)      /* HIP runtime error                 -> RuntimeError */
#define BT_ERR_WORKSPACE (-3)/* workspace too small               -> RuntimeError */

#define BT_PREC_F32 0  /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 activations: float16=False */
#define BT_PREC_HALF 1 /* half-precision MFMA operands (IEEE fp16; bfloat16 in a -DBT_HALF_BF16 build, see bt_half_is_bf16),
                        * fp32 accumulate + fp32 residual stream: float16=True */
/* (2 was BT_PREC_FP8, an experimental e4m3 feed-forward path of rounds 1-2: withdrawn in round 3 -- on every golden case
 * its logit error stayed far above the reference's own reduced-precision error and it was no faster) */

#define BT_PREC_F32X3 3 /* fp32-class results at half-MFMA speed -- the precision that carries the 1e-3 / identical-beats gate:
                        * every fp32 operand of every product (QKV, attention scores, P.V, out-projection, feed-forward,
                        * convolutions, frontend.linear) is a hi + lo pair of IEEE fp16 halves (a = hi + lo to 2^-22) and
                        * a.b ~ lo.hi + hi.lo + hi.hi on three half MFMAs, fp32 accumulate: 16/3 times the fp32 matrix rate.
                        * Residual stream, statistics, softmax sums, GELU (exact erf form), stem and head stay fp32.
                        * Activations travel between kernels as interleaved hi / lo half planes ("hl32": per 32 consecutive
                        * columns 32 hi halves then 32 lo halves), weights come packed the same way (bt_pair_weights.w_*_x3;
                        * where they are NULL or a shape does not fit, the GEMM falls back to the register-staged kernel on
                        * [hi | lo] weights, beat_this_amd/pack.py _mat).  IEEE fp16 builds only.
                        * RANGE: a hi part holds |a| <= 65504 (main layers, like the reference's own fp16 autocast) or
                        * |a| <= 1023 (register-chained frontend halves, whose operands are pre-scaled by 64).  Beyond that a
                        * split yields inf, and inf / NaN then spreads to every token of the chunk (attention).  The first
                        * int32 of the workspace is the forward's range flag: bt_forward zeroes it; the gemm3 / attention /
                        * QKV kernels OR 1 into it when a value beyond 65504 goes through a split, and whatever ends the call
                        * -- the head (logits), the final norm or the frontend's exit (bt_forward_stages with last < 2) --
                        * ORs 2 when its output is not finite, which covers the splits that do not test their operands (the
                        * register-chained frontend halves, the register-staged GEMM).  A caller that finds the word non-zero
                        * after the forward must repeat the batch in BT_PREC_F32 (beat_this_amd/pack.py: Engine does). */

#define BT_MAX_LAYERS 32

typedef struct bt_engine bt_engine;

/* One [RMSNorm -> gated RoPE attention -> +x ; RMSNorm -> FF -> +x] pair
 * (roformer.py:38-61,83-132,176-179).  Weight matrices come in two device copies,
 * index BT_PREC_F32 / BT_PREC_HALF, row-major [N padded to a multiple of 128][K]:
 *   w_qkvg : rows = q (heads*32, scaled by log2(e)/sqrt(32)) | k | v | gate rows (heads),
 *            every row multiplied by the attention RMSNorm gamma;
 *   w_out  : to_out.0.weight;  w_ff1 : net.1.weight * FF gamma;  w_ff2 : net.4.weight. */
typedef struct {
  int32_t dim, heads;
  const void* w_qkvg[2];
  const float* b_gates;
  const void* w_out[2];
  const void* w_ff1[2];
  const float* b_ff1;
  const void* w_ff2[2];
  const float* b_ff2;
  /* ("PERM32" below: columns reordered inside every block of 32, new[16 g + r] = old[(r & 3) + 8 (r >> 2) + 4 g],
   * g in {0,1}, r in [0,16) -- the order in which an MFMA accumulator holds them.)
   * FF weights for ff_fused_kernel, fragment-major: for each hidden block hb (32 hidden units):
   * dim/32 tiles of W1 (rows hb*32.., k-tile kt) then dim/32 tiles of PERM32'd W2 (rows mt*32..,
   * cols hb*32..); a tile is [half h][lane 0..63][8] (bf16) or [quarter][lane][4] (fp32) with
   * element (lane, i) = W[tile_row0 + (lane & 31)][tile_col0 + 16 (lane >> 5) + i], i in [0,16). */
  const void* w_ff_frag[2];
  /* bf16 QKV+gate weights for qkv_front_kernel (time-direction attention of the frontend, dim <= 128),
   * fragment-major tiles [half h][lane][8] as above, in the order: for every head hd the dim/32 k-tiles
   * of its 32 q rows, then of its k rows, then of its v rows; after the last head dim/32 tiles of the
   * gate rows (w_qkvg rows 3 dim .. 3 dim + 31).  NULL for dim > 128. */
  const void* w_qkv_frag;
  /* Weights of the fused out-projection + FF kernels (csrc/fused2.hip), fragment-major tiles as above, two
   * precisions, uniform steps of 2 dim/32 tiles: per 32-row block mt of to_out.0.weight its dim/32 k-tiles
   * (natural k order) + as many zero tiles, then
   * the w_ff_frag stream with W1's columns PERM32-ordered as well.  NULL for dim > 128. */
  const void* w_outff_frag[2];
  /* Weights of the fused frequency-direction kernel (attention + FF), fragment-major, steps of 2 dim/32 tiles:
   * [gate rows of w_qkvg | zero tiles], per head [q rows | k rows] [v rows | PERM32'd to_out tiles (row block
   * mt, the head's 32 columns)], then the FF steps as in w_outff_frag.  NULL for dim > 128. */
  const void* w_attnff_frag[2];
  /* Weights of the fused layer tail (csrc/tail.hip: x += to_out(ao); x += FF(x) in one launch; main layers with
   * dim = 256 / 512, half precision only; NULL elsewhere): fragment-major tiles [half h][lane][8] as above, steps of
   * 2 dim/32 tiles: for st = 0 .. dim/64 - 1 the dim/32 k-tiles of to_out.0.weight's row block 2 st, then of row block
   * 2 st + 1 (natural k order); then for i = -1 .. hidden/32 the step [A(i + 1) | B(i - 1)], A(j) = the dim/32 k-tiles of
   * (net.1.weight * FF gamma) rows 32 j .. (k columns PERM32-ordered), B(j) = the dim/32 row tiles of net.4.weight's
   * columns 32 j .. (PERM32-ordered inside the block); halves that do not exist (j < 0, j >= hidden/32) are zero tiles. */
  const void* w_tail_frag;
  /* BT_PREC_F32X3 forms of w_outff_frag / w_attnff_frag: the half fragment stream of 64 x the weight's hi part and of
   * its lo part, interleaved per 32 x 32 tile ([hi tile 2 KB | lo tile 2 KB]).  NULL: the fp32 kernels run instead. */
  const void* w_outff_frag_x3;
  const void* w_attnff_frag_x3;
  /* BT_PREC_F32X3 on the LDS-DMA kernels (csrc/gemm3.hip, csrc/qkv_front.hip): the four matrices as hl32 half arrays
   * [N padded to 256][2 K] (per 32 columns the 32 hi halves, then the 32 lo halves of w - hi), and the hi / lo fragment
   * stream of w_qkv_frag in the layout of w_outff_frag_x3 (64 x the weight).  NULL: the register-staged GEMM runs. */
  const void* w_qkvg_x3;
  const void* w_out_x3;
  const void* w_ff1_x3;
  const void* w_ff2_x3;
  const void* w_qkv_frag_x3;
  /* BT_OPT_X3_GEMM_FP8 (BASELINE config 5): the four matrices of w_*_x3 as "hl8" half arrays [N padded to 256][2 K] -- per 32
   * columns 32 hi halves, 32 hi bytes e4m3(w), 32 lo bytes e4m3(2^11 (w - hi)): 128 B like an hl32 group.  NULL: the hl32
   * form runs for that GEMM.  (An hl8 ACTIVATION, written by the kernels for each other, carries 2^-3 of that in its byte
   * sections -- e4m3(a / 8), e4m3(2^8 (a - hi)) -- so that it reaches |a| = 3584 where e4m3 alone ends at 448; beyond it the
   * producer raises the range flag.) */
  const void* w_qkvg_f8;
  const void* w_out_f8;
  const void* w_ff1_f8;
  const void* w_ff2_f8;
} bt_pair_weights;

/* Packed BeatThis weights (beat_tracker.py:38-106).  Host-side packing is done by
 * beat_this_amd/pack.py from a reference-layout state dict. */
typedef struct {
  int32_t transformer_dim, n_layers, sum_head, partial_transformers;
  /* stem (beat_tracker.py:108-126): BN1d as scale/shift per mel bin; conv weight
   * [32][df*3+dt] with BN2d scale folded; BN2d shift as bias. */
  const float* bn1_scale;
  const float* bn1_shift;
  const float* stem_w;
  const float* stem_b;
  bt_pair_weights front[3][2];  /* [block][0 = frequency direction, 1 = time direction] */
  /* frontend convs (beat_tracker.py:155-166): [2C padded][3 taps * 2 freq * C] with BN folded */
  const void* conv_w[3][2];
  const float* conv_b[3];
  /* frontend.linear (beat_tracker.py:76-77), columns permuted from (c f) to (f c) */
  const void* lin_w[2];
  const float* lin_b;
  bt_pair_weights layers[BT_MAX_LAYERS];
  const float* head_w; /* [2][D] task_heads weight * final RMSNorm gamma */
  float head_b[2];
  const float* rope;   /* [rope_len][16][2] cos/sin of pos * freqs (rotary-embedding-torch), fp32 products like the reference's */
  int32_t ff_mult;     /* hidden width of the main layers' FeedForward = ff_mult * transformer_dim (the frontend's partial
                        * transformers always use 4, beat_tracker.py:279,288) */
  /* for bt_forward_stages only: the final RMSNorm's gamma [D] and the task_heads weight [2][D] without it */
  const float* norm_out_g;
  const float* head_w_raw;
  /* BT_PREC_F32X3: hl32 forms (see bt_pair_weights.w_qkvg_x3) of conv_w / lin_w; NULL: the register-staged GEMM runs */
  const void* conv_w_x3[3];
  const void* lin_w_x3;
  int32_t rope_len;    /* rows of `rope` = the longest sequence (frames per item) bt_forward accepts; 0 means 1536 */
} bt_model_desc;

typedef struct {
  const float* window;   /* [1024] periodic Hann */
  const float* twiddle;  /* [1089][2]  (see csrc/logmel.hip) */
  const int32_t* mel_start; /* [128] first FFT bin of each mel filter */
  const int32_t* mel_len;   /* [128] */
  const float* mel_w;       /* [128][32], 16-byte aligned; a row is ZERO beyond the filter's mel_len (the kernel reads it four taps at a time) */
} bt_logmel_tables;

const char* bt_last_error(void);
/* ABI version of this header: bumped whenever an entry point's signature, a struct layout or a BT_PREC_* value changes; a
 * binding must see exactly the value it was written against (beat_this_amd/_lib.py does) */
#define BT_ABI_VERSION 600
int bt_version(void);
/* operand type of the half-precision path (BT_PREC_HALF slot of the weight arrays) this library was built
 * with: 0 = IEEE fp16 (default), 1 = bfloat16 (-DBT_HALF_BF16) */
int bt_half_is_bf16(void);
/* sizeof/offsetof of the structs above as this library was compiled (binding self-check):
 * out[9] = {pair_weights, model_desc, logmel_tables, gemm_args, attn_args, offsetof layers, offsetof rope,
 * attn_frag_args, gemm3_args} */
void bt_struct_sizes(int32_t* out);

/* BeatThis(**hparams) + load_state_dict (inference.py:56-87): keeps a copy of `desc`. */
int bt_engine_create(const bt_model_desc* desc, bt_engine** out);
void bt_engine_destroy(bt_engine* e);
/* Options of an engine (arithmetic variants of BT_PREC_F32X3 that stay inside north_star's 1e-3 / identical-beats gate but
 * are not bit-identical to each other; both are kept so that the choice can be measured: tools/flip_soak.py,
 * profiles/r05_flip_frontier.txt).  bt_engine_set_option returns BT_ERR_ARG for an unknown option / value.
 *   BT_OPT_X3_ATTN_P16  the attention probabilities enter P.V as their fp16 hi parts (two MFMAs per fragment pair instead of
 *                       three), row sums from the same rounded values:  1 (default since round 6) in the main layers only;
 *                       2 in the frontend's time-direction attention as well (round 5's default: +2 % throughput, 2.7 x the
 *                       exact path's beat flips on trained-like weights over the soak -- an opt-in, not the default: the default
 *                       is chosen by the flip-soak rule of DESIGN.md section 3);  0: three-term P.V with the probabilities
 *                       split hi + lo everywhere (rounds 3 - 4);  3: P16 in the frontend only (a variant for the flip soak: which half
 *                       of the attention launches the flips come from).
 *   BT_OPT_X3_GEMM_FP8  0 (default);  BASELINE config 5 -- GEMMs of the main layers run the two cross terms of every hi + lo product
 *                       (hi . lo + lo . hi: 2^-11 of the product) on ONE block-scaled fp8 MFMA per 32-k step instead of four fp16
 *                       ones, operands travelling as hl8 (bt_pair_weights.w_*_f8): 2 MFMA units per product instead of 3.
 *                       1: the feed-forward GEMMs (FF1, FF2);  2: out-projection and QKV as well.  An opt-in speed setting inside
 *                       the 1e-3 gate, reported beside the default (bench.py: configs.cfg5; flip rates: DESIGN.md section 3):
 *                       measured at level 2 -4 % forward time, 1.7e-4 .. 2.5e-4 on the logits against the oracle (default 7e-5),
 *                       1.1 x (outlier weights) to 14 x (freshly initialised) the default's beat flips over the 96-track soak.
 *                       Activations beyond 3584 (hl8's range) raise the range flag like those beyond 65504 on the default path.
 *   BT_OPT_WS_GUARD     0 (default): the workspace regions of bt_forward / bt_forward_stages / bt_forward_unit lie back to back.
 *                       A multiple of 256: that many bytes are left unused after every region (bt_workspace_regions), and
 *                       bt_workspace_bytes (so bt_audio2beats_plan's forward_bytes) counts them -- a test sets it to see
 *                       a kernel that writes past its region.  Kernels and launches are the same for every value. */
#define BT_OPT_X3_ATTN_P16 1
#define BT_OPT_X3_GEMM_FP8 2
#define BT_OPT_WS_GUARD 3
int bt_engine_set_option(bt_engine* e, int option, int value);
int bt_engine_get_option(const bt_engine* e, int option, int* value);
/* bytes of scratch bt_forward needs for a [B,T,128] batch (its first int32 is the BT_PREC_F32X3 range flag) */
size_t bt_workspace_bytes(const bt_engine* e, int B, int T, int prec);
/* the regions bt_forward carves out of that workspace, in address order (region 0 is the 256-byte status block that holds the
 * range flag): begin_end[2 i], begin_end[2 i + 1] = byte offsets of region i's start and of the end of the bytes it asks for
 * (before the 256-byte alignment and the BT_OPT_WS_GUARD gap).  Writes at most `max` regions; returns their total count, or a
 * negative BT_ERR_* code. */
int bt_workspace_regions(const bt_engine* e, int B, int T, int prec, int64_t* begin_end, int max);

/* BeatThis.forward (beat_tracker.py:188-192): d_spect [B,T,128] fp32 ->
 * d_beat, d_downbeat [B,T] fp32 logits (SumHead applied).  Any T <= bt_model_desc.rope_len (the reference's chunks have
 * T = 1500; its module takes any length, and so does this one given a rotary table that long). */
int bt_forward(bt_engine* e, void* stream, int prec, const float* d_spect, int B, int T, void* d_ws,
               size_t ws_bytes, float* d_beat, float* d_downbeat);

/* The three stages of BeatThis.forward on their own (beat_tracker.py:188-192: x = frontend(x); x = transformer_blocks(x);
 * x = task_heads(x)), for callers that call or hook the sub-modules: stages first..last run (0 = frontend: [B,T,128] ->
 * [B,T,D]; 1 = transformer_blocks incl. its final RMSNorm: [B,T,D] -> [B,T,D]; 2 = task_heads: [B,T,D] -> logits).
 * d_in is the input of stage `first`; d_out [B,T,D] receives the output of stage `last` when last < 2, otherwise
 * d_beat / d_downbeat do.  Same kernels and workspace as bt_forward (== stages 0..2). */
int bt_forward_stages(bt_engine* e, void* stream, int prec, int first, int last, const float* d_in, int B, int T, void* d_ws,
                      size_t ws_bytes, float* d_out, float* d_beat, float* d_downbeat);

/* The sub-modules below the three stages (what a caller of the reference reaches as model.frontend.stem, .blocks[i],
 * .blocks[i].partial, .linear, model.transformer_blocks.layers[l][0] / [1], .norm -- beat_tracker.py:54-80,108-168,
 * roformer.py:138-181), one unit per call, fp32 tensors in THIS library's activation layout, on the generic kernels (not
 * the fused fast path of bt_forward): BT_PREC_F32 or BT_PREC_HALF (BT_PREC_F32X3 is taken as BT_PREC_F32).
 *   BT_UNIT_STEM     d_in spect [B,T,128]              -> d_out [B,T,32,32]   (b, t, f, c)
 *   BT_UNIT_PARTIAL  index = block: d_in [B,T,F,C]     -> d_out [B,T,F,C]     PartialFTTransformer (F = 32 >> index, C = 32 << index)
 *   BT_UNIT_CONV     index = block: d_in [B,T,F,C]     -> d_out [B,T,F/2,2C]  conv (2,3) / stride (2,1) + BatchNorm + GELU
 *   BT_UNIT_LINEAR   d_in [B,T,4,256] (= (f c) order)  -> d_out [B,T,D]
 *   BT_UNIT_ATTN     index = layer: d_in [B,T,D]       -> d_out = x + Attention(x)      (the residual form the layer computes)
 *   BT_UNIT_FF       index = layer: d_in [B,T,D]       -> d_out = x + FeedForward(x)
 *   BT_UNIT_NORM     d_in [B,T,D]                      -> d_out = RMSNorm(x)
 *   BT_UNIT_FRONT_ATTN / BT_UNIT_FRONT_FF   the four leaves of a PartialFTTransformer (beat_tracker.py:251-301: attnF, ffF, attnT,
 *                    ffT -- ordinary Attention / FeedForward modules of width C = 32 << block on "(b t) f c" / "(b f) t c" rows):
 *                    index = 2 block + direction (0 = F, 1 = T); here B = sequences, T = tokens per sequence:
 *                    d_in [B,T,C] -> d_out = x + Attention(x) / x + FeedForward(x)
 * d_out may equal d_in for the in-place units (PARTIAL, ATTN, FF, FRONT_*).  Workspace as for bt_forward. */
enum { BT_UNIT_STEM = 0, BT_UNIT_PARTIAL = 1, BT_UNIT_CONV = 2, BT_UNIT_LINEAR = 3, BT_UNIT_ATTN = 4, BT_UNIT_FF = 5, BT_UNIT_NORM = 6,
       BT_UNIT_FRONT_ATTN = 7, BT_UNIT_FRONT_FF = 8 };
int bt_forward_unit(bt_engine* e, void* stream, int prec, int unit, int index, const float* d_in, float* d_out, int B, int T,
                    void* d_ws, size_t ws_bytes);

/* split_piece + zeropad (inference.py:90-135): d_chunks[b,t,:] = d_spect[d_starts[b]+t,:] or 0 */
int bt_split_chunks(void* stream, const float* d_spect, int64_t n_frames, const int32_t* d_starts, int B, int T,
                    float* d_chunks);
/* aggregate_prediction, overlap_mode="keep_first" (inference.py:138-185) */
int bt_aggregate(void* stream, const float* d_chunk_beat, const float* d_chunk_downbeat, const int32_t* d_starts,
                 int B, int T, int border, int64_t n_frames, float* d_beat, float* d_downbeat);

/* LogMelSpect.forward (preprocessing.py:56-59): d_audio [n_samples] fp32 @22.05 kHz ->
 * d_spect [1 + n_samples/441, 128].  n_samples must exceed 512 (reflect padding). */
int bt_logmel(void* stream, const bt_logmel_tables* tables, const float* d_audio, int64_t n_samples,
              float* d_spect);

/* ---- several tracks per launch (the batch form of Audio2Beats.__call__, inference.py:269-303: one launch per stage for
 * a whole list of tracks instead of a Python loop of per-track calls; same arithmetic as the single-track entry points).
 * A DEVICE table of bt_span describes the tracks: input samples, their count, the offset of the track's output in the
 * concatenated output buffer (samples for the resampler, spectrogram rows for the log-mel), and its output count. */
typedef struct { const float* d_in; int64_t n_in; int64_t out_off; int64_t n_out; } bt_span;
/* resample every track (all at the same up / down), max_n_out = the largest n_out */
int bt_resample_batch(void* stream, const bt_span* d_tracks, int n_tracks, int64_t max_n_out, int up, int down,
                      const float* d_filter, int half_len, float* d_out);
/* log-mel of every track: n_out = 1 + n_in / 441 frames written at row out_off of d_spect; every n_in > 512 */
int bt_logmel_batch(void* stream, const bt_logmel_tables* tables, const bt_span* d_tracks, int n_tracks,
                    int64_t max_frames, float* d_spect);
/* split_piece over the concatenated spectrogram: d_chunk_table [B][4] int32 = {first source row of the chunk (may lie
 * before the piece), first row of its piece, end row of its piece, unused}, ABSOLUTE rows of d_spect; rows outside the
 * piece read as zeros */
int bt_split_chunks_batch(void* stream, const float* d_spect, const int32_t* d_chunk_table, int B, int T, float* d_chunks);
/* keep_first aggregation of all pieces: d_pieces [n_pieces][4] int32 = {first frame, end frame (absolute, of the
 * concatenated d_beat / d_downbeat), first chunk, end chunk}; chunk starts from d_chunk_table */
int bt_aggregate_batch(void* stream, const float* d_chunk_beat, const float* d_chunk_downbeat, const int32_t* d_chunk_table,
                       const int32_t* d_pieces, int n_pieces, int64_t max_frames, int T, int border, float* d_beat,
                       float* d_downbeat);

/* Audio2Frames.signal2spect's resampling step (inference.py:274-275, soxr.resample on the host in the reference):
 * rational polyphase FIR on the GPU, y[m] = sum_k x[k] h[m down + half_len - k up], d_filter = 2 half_len + 1 taps
 * (beat_this_amd/tables.py: resample_filter = up * firwin(.., 1/max(up,down), kaiser 5.0), scipy.signal.resample_poly's
 * design), n_out <= ceil(n_in up / down).  Not bit-compatible with libsoxr (parity unpinned). */
int bt_resample(void* stream, const float* d_in, int64_t n_in, int up, int down, const float* d_filter, int half_len,
                float* d_out, int64_t n_out);

/* Postprocessor.postp_minimal peak mask (postprocessor.py:93-99) + nonzero (:119-120):
 * d_logits [n_arrays][n] -> d_idx [n_arrays][n] ascending frame indices, d_count [n_arrays]. */
int bt_peaks(void* stream, const float* d_logits, int64_t n, int n_arrays, int32_t* d_idx, int32_t* d_count);
/* ragged form: array a = d_logits + d_spans[2 a], d_spans[2 a + 1] frames; its indices are written at d_idx + d_spans[2 a] */
int bt_peaks_batch(void* stream, const float* d_logits, const int32_t* d_spans, int n_arrays, int32_t* d_idx,
                   int32_t* d_count);
/* HOST: the same peak mask for logits in host memory (the reference's Postprocessor accepts CPU tensors,
 * postprocessor.py:58-83); idx must hold n entries */
int bt_peaks_host(const float* logits, int64_t n, int32_t* idx, int32_t* count);

/* DBN post-processing (Postprocessor(type="dbn"), postprocessor.py:28-37,138-173; csrc/dbn.hip): madmom's
 * DBNDownBeatTrackingProcessor restated -- one bar HMM per entry of beats_per_bar, float64 Viterbi, the `correct` step.
 *
 * bt_dbn_tables: the state / transition / observation tables of one parameter set (reference: fps 50, bpm 55..215,
 * num_tempi 60, transition_lambda 100, observation_lambda 16, threshold 0.05, beats_per_bar {3, 4}) in HOST memory.
 * tables == NULL: *bytes = the size of the blob.  Otherwise *bytes (>= that size) bytes at tables are filled; upload them
 * as they are for the device entry points.  Parameter sets the kernel cannot run (more than 255 beat intervals, more
 * than 8192 states per HMM, more than 1536 tempo transitions, more than 4 HMMs or 16 beats per bar) return BT_ERR_ARG.
 * Blob layout (little endian, no padding): int32 magic "DBN1", K (intervals), n_hmm, states per beat, nnz, reserved;
 * int32 beats[4], num_states[4]; double init[4] (log(1 / num_states)), observation_lambda - 1, threshold;
 * int32 intervals[256], first[256] (first state of each interval inside a beat), band_ptr[258], band_from[1536];
 * double logp[1536]; uint8 cnt[16][256] -- 25712 bytes.  The tempo transitions into the first state of interval j are the entries
 * band_ptr[j] .. band_ptr[j+1]-1 (from the last state of interval band_from[e] of the previous beat, log probability
 * logp[e], ascending from-interval); cnt[b][j] = the leading states of interval j in beat b whose observation pointer
 * is >= 1 (2 in beat 0, 1 elsewhere). */
int bt_dbn_tables(double fps, double min_bpm, double max_bpm, int num_tempi, double transition_lambda,
                  double observation_lambda, double threshold, const int32_t* beats_per_bar, int n_hmm, void* tables,
                  size_t* bytes);
/* device workspace of bt_dbn_decode for n_tracks tracks of total_frames frames (and of bt_dbn_viterbi: n_tracks = 1) */
size_t bt_dbn_workspace_bytes(const void* tables, int n_tracks, int64_t total_frames);
/* ragged DBN decode of n_tracks tracks: track k's beat logits at d_logits[d_spans[4 k]], its downbeat logits at
 * d_logits[d_spans[4 k + 1]], d_spans[4 k + 2] frames each, d_spans[4 k + 3] = the frames of the tracks before it
 * (total_frames = their sum).  d_logits: float32, or float64 when f64 = 1.  tables: the host blob, d_tables: its device
 * copy.  d_out (n_tracks + 2 total_frames int32): d_out[k] = row count of track k, its rows (frame, beat number in the
 * bar; 1 = downbeat) at d_out + n_tracks + 2 d_spans[4 k + 3].  Three launches on the stream, no synchronisation. */
int bt_dbn_decode(void* stream, const void* tables, const void* d_tables, const void* d_logits, int f64,
                  const int32_t* d_spans, int n_tracks, int64_t total_frames, int32_t* d_out, void* d_ws, size_t ws_bytes);
/* the Viterbi of HMM `hmm` alone on given log densities d_dens [n][3] (observation pointer 0, 1, 2): d_path [n] state
 * indices (left untouched when *d_log_prob is -inf), d_log_prob the path's log probability */
int bt_dbn_viterbi(void* stream, const void* tables, const void* d_tables, int hmm, const double* d_dens, int64_t n,
                   int32_t* d_path, double* d_log_prob, void* d_ws, size_t ws_bytes);
/* HOST: the same recursion in C++ (bit-identical: same fp64 operations in the same order) */
int bt_dbn_viterbi_host(const void* tables, int hmm, const double* dens, int64_t n, int32_t* path, double* log_prob);
/* HOST: DBN decode of one track whose logits live in host memory (float64; rows as bt_dbn_decode, at most n of them) */
int bt_dbn_host(const void* tables, const double* beat, const double* downbeat, int64_t n, int32_t* rows, int32_t* n_rows);
/* HOST: the same from a combined activation act [n][2] (madmom's processor input: beat-not-downbeat, downbeat) */
int bt_dbn_host_act(const void* tables, const double* act, int64_t n, int32_t* rows, int32_t* n_rows);

/* Beat-tracking metrics (the reference's Metrics, pl_module.py:320-339, behind launch_scripts/compute_paper_metrics.py;
 * csrc/metrics.hip): mir_eval.beat's trim_beats, f_measure, cemgil and continuity restated from mir_eval's published
 * algorithm (0.7 / 0.8: beat.py trim_beats, validate, _get_reference_beat_variations, f_measure, cemgil, continuity;
 * util.py match_events, _fast_hit_windows, f_measure, validate_events), fp64 throughout.  Not pinned against mir_eval.
 *
 * Tracks come in CSR form: track k's reference beats are ref[ref_off[k] .. ref_off[k + 1]), its estimates
 * est[est_off[k] .. est_off[k + 1]) (int64 offsets, n_tracks + 1 of each).  Both are trimmed to the events >= min_beat_time
 * (trim_beats; -INFINITY keeps all), then scored with the match window f_window (reference 0.07 s), cemgil_sigma (0.04 s)
 * and the continuity thresholds phase_thr / period_thr (0.175, 0.175).  Output: n_tracks rows of BT_METRICS_COLS doubles
 *   F, P, R, Cemgil, CemgilMax, CMLc, CMLt, AMLc, AMLt, n_ref_trimmed, n_est_trimmed, status
 * (F, Cemgil, CMLc .. AMLt as mir_eval returns them; P and R the precision and recall behind F).  status 0: a valid track.
 * Otherwise the OR of BT_METRICS_* bits (reference array; << 3 for the estimates) and the 9 metrics are NaN: where
 * mir_eval's validate raises (an event not finite, a kept event after 30000 s, kept events decreasing; the kept events must
 * be a suffix of the array, as they are in any sorted one), unusable offsets, or -- device only -- estimates whose nearest
 * annotation is not monotone (distinct events closer than the rounding of their distances; bt_beat_metrics_host scores those). */
#define BT_METRICS_COLS 12
#define BT_METRICS_NONFINITE 1
#define BT_METRICS_UNSORTED 2
#define BT_METRICS_LATE 4
#define BT_METRICS_NEAREST 64
#define BT_METRICS_OFFSETS 128
/* device workspace of bt_beat_metrics (today it depends on n_tracks only) */
size_t bt_beat_metrics_workspace_bytes(int n_tracks, int64_t total_ref, int64_t total_est);
/* ragged metrics of n_tracks tracks, all pointers device memory, d_out n_tracks x BT_METRICS_COLS doubles.  Two launches on the
 * stream, no synchronisation. */
int bt_beat_metrics(void* stream, const double* d_ref, const int64_t* d_ref_off, const double* d_est, const int64_t* d_est_off,
                    int n_tracks, double min_beat_time, double f_window, double cemgil_sigma, double phase_thr,
                    double period_thr, void* d_ws, size_t ws_bytes, double* d_out);
/* HOST: the same rows from host memory, by mir_eval's sequential loops (Cemgil may differ from the device's in the last bits:
 * the device sums in a tree and its exp is not glibc's; every other column is bit-identical) */
int bt_beat_metrics_host(const double* ref, const int64_t* ref_off, const double* est, const int64_t* est_off, int n_tracks,
                         double min_beat_time, double f_window, double cemgil_sigma, double phase_thr, double period_thr,
                         double* out);

/* The rest of mir_eval.beat: goto, p_score and information_gain (mir_eval 0.7's beat.py restated; csrc/metrics.hip and the
 * DESIGN.md section on the extended metrics; not pinned against mir_eval).  Input, trimming, validation and the status bits
 * are bt_beat_metrics's.  goto_threshold / goto_mu / goto_sigma (mir_eval: 0.35, 0.2, 0.2), p_score_threshold (0.2), bins
 * (41; 1 .. 1024, else BT_ERR_ARG).  Output: n_tracks rows of BT_METRICS_EXT_COLS doubles
 *   Goto, PScore, InfoGain, GotoCriteria, GotoTrackLen, GotoMean, GotoStd, PWindow, PHits, EntropyFwd, EntropyBwd, status
 * Goto is 0.0 or 1.0; columns 3 .. 10 are the quantities behind the three metrics: goto's criteria (0, 1 or 3), the length
 * of its slice `track` (0: none), mean(abs(track)) and std(track, ddof = 1) (NaN for no track, an empty one or, the std, one
 * element), p_score's win_size and the integer sum of its truncated correlation, and the two entropies of information_gain.
 * A metric that returns early (an empty side for goto, fewer than two beats on a side for the others) writes 0 there.
 * A non-zero status of bt_beat_metrics's kinds makes columns 0 .. 10 NaN.  BT_METRICS_PSCORE alone: both sides have two or
 * more kept beats but every kept reference beat falls into one 10 ms index, where mir_eval's p_score raises ValueError (the
 * median of no intervals); then only columns 1, 7 and 8 are NaN. */
#define BT_METRICS_EXT_COLS 12
#define BT_METRICS_PSCORE 256
/* device workspace of bt_beat_metrics_ext (it depends on n_tracks only) */
size_t bt_beat_metrics_ext_workspace_bytes(int n_tracks, int64_t total_ref, int64_t total_est);
/* all pointers device memory, d_out n_tracks x BT_METRICS_EXT_COLS doubles.  Two launches on the stream, no synchronisation;
 * two calls on the same input give the same bits. */
int bt_beat_metrics_ext(void* stream, const double* d_ref, const int64_t* d_ref_off, const double* d_est,
                        const int64_t* d_est_off, int n_tracks, double min_beat_time, double goto_threshold, double goto_mu,
                        double goto_sigma, double p_score_threshold, int bins, void* d_ws, size_t ws_bytes, double* d_out);
/* HOST: the same rows from host memory by mir_eval's sequential loops (p_score by counting pairs of distinct indices).
 * GotoMean, GotoStd, the entropies and InfoGain may differ from the device's in the last bits (sums in another order, another
 * log2); the other columns are bit-identical unless a Goto mean or std lies within that rounding of its threshold. */
int bt_beat_metrics_ext_host(const double* ref, const int64_t* ref_off, const double* est, const int64_t* est_off, int n_tracks,
                             double min_beat_time, double goto_threshold, double goto_mu, double goto_sigma,
                             double p_score_threshold, int bins, double* out);

/* Training losses (the reference's beat_this/model/loss.py: MaskedBCELoss, ShiftTolerantBCELoss, SplittedShiftTolerantBCELoss;
 * csrc/loss.hip) with their gradients in the logits.  Rows come in CSR form: row r is elements
 * offsets[r] .. offsets[r + 1] of logits, targets and mask (int64 offsets, n_rows + 1 of them; a (B, T) batch has equal
 * steps).  kind BT_LOSS_*; tolerance in [0, BT_LOSS_MAX_TOLERANCE] (ignored by the masked loss); a row of T frames has
 * T - 4 tolerance output frames (T for the masked loss) and needs T >= 1 + 4 tolerance.  Element types BT_LOSS_F32 / _F16 /
 * _BF16 for the logits, _F32 / _F16 for the targets, _F32 / _U8 (bool) for the mask (mask NULL: all ones).  Terms are
 * evaluated in fp32 (torch's formula with pos_weight) and summed in fp64, each row by segments of BT_LOSS_SEGMENT frames with
 * fixed trees: the bits of a row do not depend on the other rows or the launch geometry. */
#define BT_LOSS_MASKED 0
#define BT_LOSS_SHIFT_TOLERANT 1
#define BT_LOSS_SPLITTED 2
#define BT_LOSS_F32 0
#define BT_LOSS_F16 1
#define BT_LOSS_BF16 2
#define BT_LOSS_U8 3
#define BT_LOSS_MAX_TOLERANCE 32
#define BT_LOSS_SEGMENT 256
/* device workspace of bt_bce_loss for n_rows rows of at most max_len frames (0: arguments out of range) */
size_t bt_bce_loss_workspace_bytes(int n_rows, int64_t max_len);
/* the loss of a ragged batch, all pointers device memory.  min_len / max_len: bounds of the rows' lengths the caller knows on
 * the host (checked against the tolerance here; a row outside them gets a NaN sum and count -1 on the device).  pos_weight, or
 * the fp32 scalar at d_pos_weight when that is not NULL.  Outputs, each optional: d_row_sum (n_rows doubles: the row's sum of
 * weighted terms), d_row_count (n_rows int64: its output frames), d_loss (one scalar of loss_dtype: the sum over all rows
 * divided by the count over all rows, the reference's mean), d_grad (fp32 per element: d(row sum)/d(logit), 0 where no window
 * takes the frame), d_terms (fp32 per element: the frame's weighted term, 0 outside the output frames).  Two launches on the
 * stream, no synchronisation, no atomics. */
int bt_bce_loss(void* stream, int kind, int tolerance, float pos_weight, const float* d_pos_weight, const void* d_logits,
                int logit_dtype, const void* d_targets, int target_dtype, const void* d_mask, int mask_dtype,
                const int64_t* d_offsets, int n_rows, int64_t min_len, int64_t max_len, void* d_ws, size_t ws_bytes,
                double* d_row_sum, int64_t* d_row_count, void* d_loss, int loss_dtype, float* d_grad, float* d_terms);
/* backward of the mean: d_grad_in[i] = d_grad[i] * (*d_grad_output / count), written as grad_in_dtype (BT_LOSS_F32 / _F16 /
 * _BF16); d_grad_output is one scalar of grad_output_dtype in device memory.  One launch, no synchronisation. */
int bt_bce_loss_backward(void* stream, const float* d_grad, int64_t n, const void* d_grad_output, int grad_output_dtype,
                         int64_t count, void* d_grad_in, int grad_in_dtype);
/* HOST: the same from host memory, with the same fp32 terms, gathers and fp64 trees (row sums, terms and gradients bit-identical
 * to the device's); *total (optional) = the mean.  Rows shorter than 1 + 4 tolerance are refused with BT_ERR_ARG. */
int bt_bce_loss_host(int kind, int tolerance, float pos_weight, const void* logits, int logit_dtype, const void* targets,
                     int target_dtype, const void* mask, int mask_dtype, const int64_t* offsets, int n_rows, double* row_sum,
                     int64_t* row_count, double* total, float* grad, float* terms);

/* Training batches (the reference's beat_this/dataset: BeatTrackingDataset.__getitem__ + collate; csrc/data.hip, DESIGN.md
 * section 12): excerpts of a resident spectrogram store with the mask augmentation applied as a gather, the framewise
 * targets and the masks, ONE launch per batch, no memset, no atomics, no synchronisation, no allocation.
 *
 * Store: [store_rows][128] of store_dtype (BT_LOSS_F16 / BT_LOSS_F32).  Item b takes n <= L frames from store row `row`
 * on; output frame t >= n is padding (zero spectrogram, zero targets, padding mask 0).  Its mask ops are ops[op_begin ..
 * op_end) in the order the reference applies them in place; output frame t is resolved by walking them from the LAST to the
 * first: outside [start, start + length) t stays; inside a BT_MASK_ZERO op the frame is zero; inside a BT_MASK_PERMUTE op
 * t = start + old_off + (t - start - new_off) of the last part (parts[part_begin .. part_end), ascending new_off, new_off[0]
 * = 0, no empty parts) whose new_off <= t - start.  Its annotations are time / value [ann_begin .. ann_end), times
 * ascending; annotation i lies on frame rint(time[i] * fps) - start_frame (fp64, ties to even) and counts when
 * 0 <= frame < n; it is a downbeat when value[i] == 1.  downbeat_mask[b] = has_downbeats != 0. */
#define BT_MASK_ZERO 0
#define BT_MASK_PERMUTE 1
#define BT_TRAIN_FRAME_BLOCK 64   /* frames per workgroup */
typedef struct {
  int64_t row;                 /* first store row of the excerpt */
  int64_t ann_begin, ann_end;  /* its range in the annotation arrays */
  int32_t n;                   /* frames of the excerpt, 0 <= n <= L */
  int32_t start_frame;         /* frame of the piece the excerpt starts at */
  int32_t op_begin, op_end;    /* its range in the op table */
  int32_t has_downbeats;
  int32_t reserved;
} bt_train_item;
typedef struct {
  int32_t start, length, kind; /* frames [start, start + length) of the excerpt, BT_MASK_* */
  int32_t part_begin, part_end;/* its range in the parts table (permute only) */
} bt_train_op;
typedef struct {
  int32_t new_off, old_off;    /* offset of the part in the permuted order and in the original one */
} bt_train_part;
/* sizeof of the three structs, then offsetof ann_begin, n, op_begin, has_downbeats (item), kind, part_begin (op), old_off
 * (part): ten entries, the binding's self-check */
void bt_train_batch_struct_sizes(int32_t* out);
/* All pointers device memory; the tables may be NULL when their count is 0.  Outputs, each optional: d_spect [B][L][128] of
 * spect_dtype (BT_LOSS_F32 / _F16; fp32 -> fp16 rounds to nearest even), d_truth_beat / d_truth_downbeat / d_padding_mask
 * [B][L] uint8 (0 / 1), d_downbeat_mask [B] uint8.  Every byte of every output given is written.  A table entry that points
 * outside its table or outside the store yields zeros, never an access outside; bt_train_batch_host refuses such tables. */
int bt_train_batch(void* stream, const void* d_store, int store_dtype, int64_t store_rows, const bt_train_item* d_items, int B,
                   int L, const bt_train_op* d_ops, int n_ops, const bt_train_part* d_parts, int n_parts,
                   const double* d_ann_time, const int32_t* d_ann_value, int64_t n_ann, double fps, void* d_spect,
                   int spect_dtype, uint8_t* d_truth_beat, uint8_t* d_truth_downbeat, uint8_t* d_padding_mask,
                   uint8_t* d_downbeat_mask);
/* HOST: the same from host memory, bit-identical outputs; tables are validated (BT_ERR_ARG names the first bad entry) */
int bt_train_batch_host(const void* store, int store_dtype, int64_t store_rows, const bt_train_item* items, int B, int L,
                        const bt_train_op* ops, int n_ops, const bt_train_part* parts, int n_parts, const double* ann_time,
                        const int32_t* ann_value, int64_t n_ann, double fps, void* spect, int spect_dtype, uint8_t* truth_beat,
                        uint8_t* truth_downbeat, uint8_t* padding_mask, uint8_t* downbeat_mask);

/* HOST: deduplicate_peaks(peaks, width) on its own (postprocessor.py:176-197): groups of ascending frame indices not more than
 * `width` apart (measured from the running mean) are replaced by their mean; out must hold n doubles */
int bt_deduplicate_peaks_host(const int32_t* idx, int n, double width, double* out, int32_t* n_out);
/* HOST: deduplicate_peaks(width=1) (postprocessor.py:176-197), frame/fps, snap every
 * downbeat to the nearest beat, np.unique (postprocessor.py:121-136).  Output buffers
 * must hold n_beat_idx / n_down_idx doubles. */
int bt_postprocess_host(const int32_t* beat_idx, int n_beat_idx, const int32_t* down_idx, int n_down_idx,
                        double fps, double* beats, int32_t* n_beats, double* downbeats, int32_t* n_downbeats);

/* Audio2Beats.__call__ for ONE track in ONE call (inference.py:269-281,301-303 without the audio decoder and the host
 * post-processing): resample (when up != down) -> log-mel -> split_piece -> BeatThis.forward -> keep_first aggregation -> peak
 * mask -> ONE device-to-host copy of the result, all enqueued on `stream` by this function -- the host language is not in the
 * loop between the stages (single-file latency, BASELINE config 1; round 5: five places where the GPU waited for Python).
 * bt_audio2beats_plan sizes the call: a track of n_in samples at a rate with 22050 / rate = up / down in lowest terms gives
 * n22 samples at 22.05 kHz, n_frames = 1 + n22 / 441 spectrogram rows and B chunks of T frames (T = 1500, or n_frames + 12 for a
 * piece of <= 1488 frames); ws_bytes of device scratch; result_words int32 of PINNED host memory:
 *     h_result = [beat peak frames: n_frames slots | downbeat peak frames: n_frames slots | n_beat, n_down | range flag]
 * (ascending frame indices as bt_peaks writes them, then the two counts, then the BT_PREC_F32X3 range flag of the forward: non-zero
 * = repeat the call with BT_PREC_F32), valid once `stream` has drained.  d_audio: mono fp32 on the device (the caller's mono mix
 * and upload).  use_graph != 0: the forward's launches are replayed as a hipGraph the engine captures itself on first use and keeps
 * per (B, T, precision, d_ws) -- d_ws must then be the same allocation from call to call (T == 1500 and B <= 16 only; other shapes
 * launch plainly).  Same kernels in the same order as the separate entry points: bit-identical results.  Framewise logits of the
 * call stay readable in d_ws at plan.off_logits ([beat n_frames | downbeat n_frames] fp32) until the next call on d_ws. */
typedef struct {
  int64_t n22, n_frames, result_words;
  int32_t B, T;
  size_t ws_bytes, off_wave22, off_spect, off_chunks, off_chunk_logits, off_logits, off_result, off_forward, forward_bytes;
} bt_a2b_plan;
int bt_audio2beats_plan(const bt_engine* e, int64_t n_in, int up, int down, int prec, bt_a2b_plan* plan);
int bt_audio2beats_enqueue(bt_engine* e, void* stream, int prec, const bt_logmel_tables* tables, const float* d_audio, int64_t n_in,
                           int up, int down, const float* d_filter, int half_len, void* d_ws, size_t ws_bytes, int32_t* h_result,
                           int use_graph);

/* Per-launch timing of bt_forward with HIP events recorded on the caller's stream (bench.py's
 * roofline leg); per engine handle.  bt_profile_begin(e) arms it; every bt_forward(e, ...) until bt_profile_end(e, ...)
 * records one event pair per kernel launch; bt_profile_end() synchronises on the events and returns summed
 * milliseconds and launch counts per category (index = BT_CAT_*). */
#define BT_CAT_STEM 0
#define BT_CAT_QKV_GEMM 1
#define BT_CAT_ATTN_FLASH 2  /* time-direction + main attention */
#define BT_CAT_OUT_GEMM 3
#define BT_CAT_FF1_GEMM 4
#define BT_CAT_FF2_GEMM 5
#define BT_CAT_CONV_GEMM 6
#define BT_CAT_LINEAR_GEMM 7
#define BT_CAT_HEAD 8
#define BT_CAT_FF_FUSED 9         /* ff_fused_kernel (frontend FF blocks) */
#define BT_CAT_ATTN_FREQ_FUSED 10 /* attnff_fused_kernel: frequency-direction half (QKV + attention + out-proj + FF) */
#define BT_CAT_LAYER_TAIL 11      /* layer_tail_kernel (main layers: out-projection + FF1 + FF2 in one launch) */
#define BT_PROFILE_CATEGORIES 12
void bt_profile_begin(bt_engine* e);
int bt_profile_end(bt_engine* e, double* ms_by_category, int32_t* launches_by_category, int n_categories);

/* Single-operator entry points (used by the parity tests; same kernels bt_forward launches). */
typedef struct {
  const void* A; int64_t lda; const void* W; int32_t M, N, K; int32_t epi, flags;
  const float* bias; void* out; int64_t ldo; float* x; int64_t ldx;
  int32_t conv_C2, conv_T, conv_F;
  float* gates; int32_t inner, heads; const float* rope; int32_t pdiv, pmod, map_T, map_F;
} bt_gemm_args;
int bt_gemm(void* stream, int prec, const bt_gemm_args* a);

typedef struct {
  const void* qkv; int64_t ld; const float* gates; void* out;
  int32_t n_seq, L, heads, inner, o_div; int64_t o_outer, o_inner, o_tok;
} bt_attn_args;
int bt_attention(void* stream, int prec, const bt_attn_args* a);

/* half-precision attention on FRAGMENT-MAJOR operands (csrc/attn2.hip): per (sequence, head) `nbp` blocks of
 * 32 tokens, 2 KB each.  Q/K block: [quarter a][token][8 dims 8a..8a+7]; V block: [s][lane = 32 g + d]
 * [8 tokens 16 s + 8 (j >> 2) + 4 g + (j & 3)]; gates [n_seq * heads][nbp * 32] fp32.  q must be
 * pre-scaled by log2(e)/sqrt(32).  nbp >= bt_attn_frag_blocks(L).  Output as bt_attention (half).
 * x3 <= 0 (half operands): 0 / -1 = the 128-query kernel (what the forward runs); -2 = two query blocks per wave on a
 * hand-scheduled key loop (round 6: same bits for every query, 2.7 % slower at 0.9 % fewer joules -- the fp16 attention is
 * bound by its exponentials; kept for tests and probes).
 * x3 > 0 (BT_PREC_F32X3): blocks of 4 KB = [hi block | lo block] of the fp32 values, three MFMAs per product; output
 * fp32 [rows, inner] (out_f32 = 1), hl32 half [rows, 2 inner] (0) or hl8 rows of the same size (2: per 32 columns 32 hi halves |
 * 32 e4m3 bytes of value / 8 | 32 e4m3 bytes of 2^8 (value - hi), what bt_gemm3 reads as A with x3 flag 0x100); status (may be NULL) =
 * range flag of the hl32 / hl8 output;
 * x3 = 1: 128-key LDS tiles, x3 = 2: 64-key tiles, x3 = 5: two query blocks per wave on a hand-scheduled key loop -- the same
 * arithmetic in all three, bit-identical results; x3 = 4 (the forward's choice since round 4): 5 where its 256-query
 * workgroups cost fewer per-CU rounds than the 128-query ones of 2 (launch_attn_frag), 2 otherwise.  + 8 (BT_X3_P16): the P16
 * arithmetic (BT_OPT_X3_ATTN_P16) on the same kernel choice.
 * x3 > 0 needs `scratch`: n_seq * heads * nbp int32 words (the launch's overflow map: queries whose probabilities left fp16's
 * range in the fast pass are recomputed on their row maxima by a second, gathered launch; contents undefined afterwards). */
#define BT_X3_P16 8
typedef struct {
  const void* q; const void* k; const void* v; const float* gates; void* out;
  int32_t n_seq, L, heads, inner, nbp, o_div; int64_t o_outer, o_inner, o_tok;
  int32_t x3, out_f32; int32_t* status;
  int32_t* scratch;
} bt_attn_frag_args;
/* BASELINE.json config 5 ("final0 fp8 MFMA weights ... CDNA4 fp8 attention/FFN path") at OPERATOR level, report-only: the GEMM of a
 * main layer's to_qkv / to_out / FeedForward linears (roformer.py:38-61,99-132) with both operands in the OCP MX e4m3 format --
 * d_A [M][K] and d_W [N padded to 128][K] e4m3 bytes, d_SA [M][K / 32] and d_SW [N padded to 128][K / 32] E8M0 scale bytes (value
 * = 2^(byte - 127) x element), K = 512 | 1024 | 2048, N % 64 == 0 -- on v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulation,
 * d_out fp32 [M][ldo].  No forward calls it: it is measured beside the fp16 GEMM (tools/mx8_probe.py) and its arithmetic is
 * priced on the oracle (tools/flip_soak.py sim --schemes mxfp8) -- DESIGN.md, config 5. */
int bt_gemm_mx8(void* stream, const void* d_A, const void* d_SA, const void* d_W, const void* d_SW, float* d_out, int M, int N,
                int K, int64_t ldo);

/* half GEMM of the main layers (csrc/gemm3.hip), single-operator entry for the parity tests.
 * epi 0: out[M,ldo] (half) = gelu(rms(A) W^T + bias);  epi 1: x[M,ldx] (fp32) += A W^T + bias, half shadow xb,
 * partial row sums of squares ssq_out[N/64][M];  epi 2: q|k|v|gates = rms(A) W^T with RoPE / sigmoid, written
 * fragment-major (layout of bt_attention_frag) for n_seq sequences of L tokens (M = n_seq L).
 * rms(A) uses ssq_in[ssq_parts][M] (partial row sums of squares of the fp32 source of A), NULL = no RMSNorm.
 * x3 != 0 (BT_PREC_F32X3): A half [M, 2 lda], W half [N padded to 256, 2 K], out half [M, 2 ldo], xb half [M, 2 ldx]
 * are hl32 (interleaved hi / lo planes of the fp32 values; K, lda, ldo, ldx count fp32 elements), q / k / v blocks are
 * 4 KB, epi 0 uses the exact erf GELU; status (may be NULL) = range flag.  x3 + 0x100: A and W are hl8 (see
 * bt_pair_weights.w_ff1_f8); x3 + 0x200: the activation the launch writes for the next GEMM (epi 0: out,
 * epi 1: xb) is hl8. */
typedef struct {
  const void* A; int64_t lda; int32_t M, K; const void* W; int32_t N, epi; const float* bias;
  const float* ssq_in; int32_t ssq_parts; void* out; int64_t ldo; float* x; int64_t ldx; void* xb; float* ssq_out;
  int32_t n_seq, L, nbp, heads; const float* rope; void* qf; void* kf; void* vf; float* gates; const float* b_gates;
  int32_t no_resid; /* epi 1: x = A W^T + bias, x is only written (frontend.linear) */
  /* epi 1 as the frontend convolution (beat_tracker.py:155-166, BatchNorm folded): gelu != 0 -> x = gelu(.. + bias) (tanh
   * form; exact erf form with x3), x may be NULL (shadow output xb only); conv_C2 = 2 C > 0 -> A is the (b, t, f, c)
   * activation shadow seen as [M = B T F/2, conv_C2], lda = conv_C2, K = 3 conv_C2: the rows m - conv_F, m, m + conv_F
   * (time taps t-1, t, t+1 with conv_F = F/2 rows per time step), rows with t outside [0, conv_T) read as zeros.  Needs
   * no_resid. */
  int32_t gelu, conv_C2, conv_T, conv_F;
  int32_t x3; int32_t* status;
} bt_gemm3_args;
int bt_gemm3(void* stream, const bt_gemm3_args* a);
int bt_attn_frag_blocks(int L);
int bt_attention_frag(void* stream, const bt_attn_frag_args* a);
/* Time-direction QKV projection of a frontend block: d_x [B,T,F,C] fp32 -> fragment-major q, k, v, gates
 * (prec = BT_PREC_HALF: 2 KB blocks from w_qkv_frag; BT_PREC_F32X3: 4 KB [hi | lo] blocks from w_qkv_frag_x3) */
int bt_qkv_front(void* stream, int prec, const bt_pair_weights* w, const float* d_rope, const float* d_x, int B, int T, int F,
                 void* d_q, void* d_k, void* d_v, float* d_gates, int nbp);
/* x[M,C] += FF(x) with one bt_pair_weights, dim = C <= 128 */
int bt_ff_fused(void* stream, int prec, const bt_pair_weights* w, float* d_x, int64_t M);
/* fused halves (csrc/fused2.hip): x += to_out(ao) then x += FF(x);  x += AttnF(x) then x += FF(x).
 * d_xb (may be NULL): shadow of the new x for the following convolution -- half [M, dim] (BT_PREC_HALF) or hl32 half
 * [M, 2 dim] (BT_PREC_F32X3) */
int bt_outff_fused(void* stream, int prec, const bt_pair_weights* w, const void* d_ao, float* d_x, int64_t M, void* d_xb);
int bt_attnff_fused(void* stream, int prec, const bt_pair_weights* w, const float* d_rope, float* d_x, int64_t M);
/* fused tail of a main layer (csrc/tail.hip, BT_PREC_HALF, w->dim = 256 / 512, w->w_tail_frag set): d_x [M, dim] fp32
 * += to_out(d_ao [M, dim] half), then += FF(x); optional outputs: d_xb = half copy of the new x, d_ssq_out [dim/64][M] =
 * partial row sums of squares of the new x (what the next layer's QKV projection consumes) */
int bt_layer_tail(void* stream, const bt_pair_weights* w, int hidden, const void* d_ao, float* d_x, int64_t M, void* d_xb,
                  float* d_ssq_out);

/* ---- training: forward and backward of the trunk's units and of the heads (csrc/train.hip) ------------
 * One call per unit, like bt_forward_unit: BT_UNIT_ATTN, BT_UNIT_FF, BT_UNIT_NORM (the trunk's final RMSNorm) and
 * BT_TRAIN_UNIT_HEAD.  Everything is fp32 with fp32 accumulation.  The parameters are read in the REFERENCE's layout and values,
 * straight from the nn.Parameter storage -- not the engine's packed copies:
 *   attention:  gamma = norm.gamma [dim], w1 = to_qkv.weight [3 dim, dim], w2 / b2 = to_gates.weight [dim / 32, dim] / .bias,
 *               w3 = to_out.0.weight [dim, dim], rope = the engine's [rope_len][16][2] cos / sin table
 *   FF:         gamma = net.0.gamma, w1 / b1 = net.1.weight [hidden, dim] / .bias, w2 / b2 = net.4.weight [dim, hidden] / .bias
 *   norm:       gamma = transformer_blocks.norm.gamma
 *   head:       w1 / b1 = task_heads.beat_downbeat_lin.weight [2, dim] / .bias [2]; sum_head: beat = b + d (SumHead) or b (Head)
 * Shapes: x, y, gy, gx [B T, dim] contiguous; dim a multiple of 32 from 32 to 1024 (heads of 32), hidden = ff_mult dim with
 * ff_mult 1 .. 16, 1 <= T <= rope_len (0: 1536); anything else is BT_ERR_ARG.  residual != 0: the unit is x + f(x) (attention and FF).
 * The forward writes y (head: y = beat, y2 = downbeat, each [B T]) and, for the attention, what the backward needs beside x:
 * save_o [B T, dim] (the attention output before the gate) and save_lse [B T, dim / 32] (base-2 log-sum-exp of the scaled
 * scores); everything else is recomputed.  The backward takes x, those two, the upstream gradient gy (head: gy = d beat, gy2 =
 * d downbeat, either may be NULL = zero) and OVERWRITES the gradients whose pointer is not NULL: gx, g_gamma, g_w1, g_b1, g_w2,
 * g_b2, g_w3 (shaped like the parameters).  Every byte of a gradient is written by one thread of one launch; there are no
 * atomics, and the order of every sum depends on (B, T, dim, hidden) only: results are bitwise reproducible, and a
 * sequence's gx is the same alone and inside a batch.  Weight gradients are summed over chunks of BT_TRAIN_DW_ROWS rows, bias
 * and gamma gradients over chunks of BT_TRAIN_CS_ROWS rows (partials in the workspace, added in chunk order by a second
 * launch); the attention works on blocks of BT_TRAIN_ATTN_BLOCK queries x keys.  No call synchronises, allocates or clears
 * memory: ws / ws_bytes is the caller's workspace, at least bt_train_workspace_bytes (0: unsupported shape), contents
 * undefined before and after; no launch reads workspace bytes that the same call has not written. */
#define BT_TRAIN_UNIT_HEAD 16
#define BT_TRAIN_DW_ROWS 1024
#define BT_TRAIN_CS_ROWS 64
#define BT_TRAIN_ATTN_BLOCK 64
typedef struct {
  int32_t B, T, dim, hidden, rope_len, residual, sum_head;
  int32_t operand;   /* read by bt_train_forward_mixed / bt_train_backward_mixed alone: BT_OPERAND_* (below); ignored elsewhere */
  const float* rope;
  const float* gamma; const float* w1; const float* b1; const float* w2; const float* b2; const float* w3;
  const float* x; float* y; float* y2; float* save_o; float* save_lse;
  const float* gy; const float* gy2;
  float* gx; float* g_gamma; float* g_w1; float* g_b1; float* g_w2; float* g_b2; float* g_w3;
  void* ws; size_t ws_bytes;
} bt_train_args;
/* sizeof, then offsetof rope, x, gy, gx, ws, ws_bytes: seven entries, the binding's self-check */
void bt_train_struct_sizes(int32_t* out);
size_t bt_train_workspace_bytes(int unit, int backward, int B, int T, int dim, int hidden);
int bt_train_forward(void* stream, int unit, const bt_train_args* a);
int bt_train_backward(void* stream, int unit, const bt_train_args* a);

/* ---- training: dropout in the attention and feed-forward units (csrc/dropout.h, csrc/train.hip) ---------
 * The reference's transformer drops at four places per layer (roformer.py): the attention probabilities, the output of to_out,
 * the GELU's output and the output of the feed-forward's second linear.  The *_dropout entry points take the unit calls'
 * arguments plus a bt_train_dropout; NULL, or p == 0, launches exactly what bt_train_forward / bt_train_backward launch (which
 * are these calls with NULL).  0 <= p < 1, anything else (NaN too) is BT_ERR_ARG; p > 0 with BT_UNIT_NORM or BT_TRAIN_UNIT_HEAD
 * is BT_ERR_ARG.  Masks are never stored: every kernel evaluates Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, key
 * increments 0x9E3779B9, 0xBB67AE85) for the elements it touches, and the backward must be given the p, seed and stream of
 * its forward.  THE MASK CONTRACT.  An element belongs to group g (64-bit) and word w (0 .. 3) of its site:
 *     counter = { g mod 2^32,  site << 24 | g >> 32,  stream mod 2^32,  stream >> 32 },  key = { seed mod 2^32, seed >> 32 }
 *     kept iff word w of Philox4x32-10(counter, key) >= thr,  thr = floor(p 2^32) computed in double (p = 0 keeps everything);
 *     a kept value is multiplied by 1 / (1 - p), computed and applied in fp32.
 *   BT_DROP_ATTN_P    [B][H][T][T], query q by key k of head h = dim / 32 of sequence b:
 *                     g = ((b H + h) T + q) ((T + 3) / 4) + k / 4,  w = k mod 4   (integer divisions; a group never leaves its
 *                     query; the words behind key T - 1 of a query's last group are unused)
 *   BT_DROP_ATTN_OUT  [B T][dim]:     g = row (dim / 4) + col / 4,     w = col mod 4   (to_out's result, before the residual)
 *   BT_DROP_FF_HIDDEN [B T][hidden]:  g = row (hidden / 4) + col / 4,  w = col mod 4   (the GELU's result)
 *   BT_DROP_FF_OUT    [B T][dim]:     g = row (dim / 4) + col / 4,     w = col mod 4   (net.4's result, before the residual)
 * `stream` is the caller's: one value per unit call, so that two calls with one seed never share a counter (the two sites of a
 * unit share the stream and differ in the site).  With dropout the attention keeps its normaliser over every key, adds p v for
 * the kept (q, k) pairs only and stores save_o = the dropped output (before the gate); save_lse is unchanged.  The backward with
 * p > 0 needs bt_train_workspace_bytes_dropout (one more [B T, dim] region: the masked upstream gradient); the forward's
 * workspace is the same as without.
 * THE LEAVES OF THE FRONTEND.  The twelve attention / feed-forward leaves of the three partial
 * transformers are these unit calls with residual != 0 on the rows of the (b, t, f, c) activation, B sequences of T frames, F
 * frequency bins, C channels ((F, C) = (32, 32), (16, 64), (8, 128) in blocks 0, 1, 2), and their (B, T) above mean:
 *   a frequency-direction leaf (attnF, ffF):  B' = B T, T' = F;  the row of token f of frame t of sequence b is (b T + t) F + f,
 *                                             sequence b' = b T + t, query / key index f
 *   a time-direction leaf (attnT, ffT):       B' = B F, T' = T;  the row of frame t of bin f of sequence b is (b F + f) T + t,
 *                                             sequence b' = b F + f, query / key index t
 * Sites, groups and words are exactly the ones above over (B', T', dim = C, hidden = ff_mult C, H = C / 32), so
 * bt_dropout_mask_host(dropout, site, B', T', C, hidden, out) gives a leaf's masks.  The streams of a whole-model forward that
 * drops in both parts, from the caller's counter n: block 0's attnF, ffF, attnT, ffT take n .. n + 3, block 1's n + 4 .. n + 7,
 * block 2's n + 8 .. n + 11, then the trunk's layer l takes n + 12 + 2 l (attention) and n + 13 + 2 l (feed-forward); a part
 * whose rate is 0, or that is not opted in, takes no number (a model without partial transformers has no leaves).  The rate
 * of the leaves is the caller's own (BeatThis: dropout["frontend"]) and may differ from the trunk's.  Dropout adds no limit:
 * every group index is 64-bit and the launches are the ones without dropout, so B' is bounded as ever by the 65535 sequences
 * of a grid (the frontend's route refuses B T > 65535 before any launch) and B' T' by 2^22 rows. */
#define BT_DROP_ATTN_P 0
#define BT_DROP_ATTN_OUT 1
#define BT_DROP_FF_HIDDEN 2
#define BT_DROP_FF_OUT 3
typedef struct {
  float p; uint32_t reserved; uint64_t seed; uint64_t stream;
} bt_train_dropout;
/* sizeof, then offsetof p, seed, stream: four entries, the binding's self-check */
void bt_train_dropout_struct_sizes(int32_t* out);
size_t bt_train_workspace_bytes_dropout(int unit, int backward, int B, int T, int dim, int hidden);
int bt_train_forward_dropout(void* stream, int unit, const bt_train_args* a, const bt_train_dropout* dropout);
int bt_train_backward_dropout(void* stream, int unit, const bt_train_args* a, const bt_train_dropout* dropout);
/* HOST: out[0 .. 3] = Philox4x32-10 of ctr[0 .. 3] under key[0 .. 1] */
void bt_philox4x32_10_host(const uint32_t* ctr, const uint32_t* key, uint32_t* out);
/* HOST: the mask of one site as bytes (1 = kept), one per element in the site's layout above; dim a multiple of 32, hidden a
 * multiple of 4 (used by BT_DROP_FF_HIDDEN only), B, T >= 1 */
int bt_dropout_mask_host(const bt_train_dropout* dropout, int site, int B, int T, int dim, int hidden, uint8_t* out);

/* ---- training: the 16-mixed route of the attention and the feed-forward (csrc/train_mixed.inc) -----------
 * The reference trains with precision="16-mixed": fp16 matrix products, fp32 master weights, a dynamic loss scale.  The *_mixed
 * entry points are the unit calls above (same bt_train_args, same bt_train_dropout or NULL, same shape limits, same saved
 * tensors x / save_o / save_lse in fp32, same recomputation, fp32 parameters read from the nn.Parameter storage, fp32 x, y, gy,
 * gx and gradients) with ONE difference.  THE ARITHMETIC CONTRACT: both operands of every matrix product are rounded to IEEE
 * fp16, round to nearest even, as they are staged, and the product accumulates in fp32 on the gfx950 fp16 MFMAs
 * (v_mfma_f32_32x32x16_f16).  The products are Y = A W^T, dA = dY W and dW = dY^T A of to_qkv, to_gates, to_out, net.1 and
 * net.4, and the attention's S = Q K^T, O = P V, dP = dO V^T, dV = P^T dO, dQ = dS K and dK = dS^T Q.  Q and K are rounded after
 * RoPE; P is rounded after the dropout mask and its 1 / (1 - p) have been applied in fp32 (in the forward P is the probability
 * relative to the running maximum of the keys seen so far, exp2(s - max), the flash form; the backward rounds exp2(s - lse)).
 * Everything else is fp32 and is the code of the fp32 route: RMSNorm and its backward, biases and residuals, the softmax
 * statistics, lse and delta, dS = P (dP - delta), the gates, the GELU and its derivative, RoPE, the column sums and the chunked
 * dW reduction (BT_TRAIN_DW_ROWS, BT_TRAIN_CS_ROWS).  A value beyond fp16's range becomes inf and propagates; nothing clamps
 * it -- the caller scales the loss and looks at the gradient norm (beat_this_amd.optim.LossScaler).
 * Kept from the fp32 route: no atomics; every gradient byte is written by one thread of one launch; every order of summation
 * depends on the shapes alone (a GEMM element sums k ascending in steps of 16, dQ its key tiles of 32 in ascending order, dK / dV
 * their query tiles of 32 in ascending order), so two runs are bit-identical; a sequence's gx is the same alone and inside a
 * batch; no launch reads workspace bytes that its own call has not written; no call synchronises, allocates or clears memory.
 * The dropout mask contract is unchanged.  Units other than BT_UNIT_ATTN and BT_UNIT_FF are BT_ERR_ARG (workspace query: 0):
 * the final norm and the head have no matrix product worth an MFMA and stay on the fp32 entries.  The workspace is that of the
 * fp32 route (with_dropout != 0: that of the dropout entries).
 * THE OPERAND FORMAT.  bt_train_args.operand -- the struct's former reserved int32, same offset -- picks the
 * 16-bit format of that contract: BT_OPERAND_F16 (0) is everything above, launch for launch.  BT_OPERAND_BF16 (1) is the same
 * contract with one word changed: both operands of every listed product are rounded to bfloat16, round to nearest even, as they
 * are staged, and accumulate in fp32 on v_mfma_f32_32x32x16_bf16.  NaN stays NaN; no value overflows by rounding (the exponent
 * range is fp32's), so this format needs no loss scale.  Staging, lane maps, summation orders, the mask mapping, the workspace
 * and everything that is kept are those of fp16.  Any other value is BT_ERR_ARG before any launch ("operand" in bt_last_error()).
 * The fp32 and dropout entry points above never read the field.
 * BT_OPERAND_BF16X3 (3; DESIGN.md section 25, "32-high") multiplies fp32 values as split bfloat16 operands.  For an fp32 value a:
 *   hi = bf16(a), rounded to nearest even;  lo = bf16(a - hi), the subtraction being exact in fp32;
 *   where hi is not finite (a is +-inf or NaN, or a finite value that rounds to inf) lo = 0 -- otherwise inf would meet -inf in
 *   the partial products and turn an overflow into NaN (3.4e38 - bf16(3.4e38) is -inf).
 * Every product listed above becomes A_lo B_hi + A_hi B_lo + A_hi B_hi; the lo lo term is dropped.  Per accumulator and per k-step
 * of 16 the three v_mfma_f32_32x32x16_bf16 are issued in that order, the small terms first, into the one fp32 accumulator.  The
 * operands that the other formats round in registers (P after mask and 1 / (1 - p), dS, the own side's fragments) are split in
 * registers.  About 2^-17 of an operand is kept where bfloat16 keeps 2^-9; the exponent range is fp32's: no range flag, no loss
 * scale, no fallback.  Everything else, every summation order, the workspace and everything that is kept are those of the other
 * formats.  Value 2 is unassigned and refused. */
#define BT_OPERAND_F16 0
#define BT_OPERAND_BF16 1
#define BT_OPERAND_BF16X3 3
size_t bt_train_workspace_bytes_mixed(int unit, int backward, int B, int T, int dim, int hidden, int with_dropout);
int bt_train_forward_mixed(void* stream, int unit, const bt_train_args* a, const bt_train_dropout* dropout_or_null);
int bt_train_backward_mixed(void* stream, int unit, const bt_train_args* a, const bt_train_dropout* dropout_or_null);
/* DIAGNOSTIC: the raw GEMM of the mixed route on fp16 operands, fp32 in and out, C [M, N] contiguous, 1 <= M, N, K <= 2^22:
 *   form 0: C = A B^T, A [M, K], B [N, K]   (Y = A W^T)
 *   form 1: C = A B,   A [M, K], B [K, N]   (dA = dY W)
 *   form 2: C = A^T B, A [K, M], B [K, N]   (dW = dY^T A; K = the summed rows, taken BT_TRAIN_DW_ROWS at a time and the chunks
 *                                            added into C in chunk order, one launch per chunk) */
int bt_train_matmul_mixed(void* stream, int form, const float* A, const float* B, int M, int N, int K, float* C);
/* The GEMM of either training route (mixed = 0: the fp32 MFMA kernels, 1: the fp16 ones, 2: the same on bfloat16 operands, 4: on
 * split bfloat16 operands -- 1 + BT_OPERAND_*; anything else, 3 included, is BT_ERR_ARG ahead of every other check) through the
 * host helpers
 * the unit calls launch it with.  A diagnostic for the trunk's units, and PRODUCTION for the frontend's projection:
 * bt_front_forward / bt_front_backward (BT_FRONT_LINEAR) call forms 0, 1 and 2 with their own `mixed` and size their workspace with
 * bt_train_matmul_workspace_bytes, so what this entry computes, and in which order it sums, is part of section 17's contract.
 * Forms as above, forms as above, C [M, N] contiguous, 1 <= M, N, K <= 2^22.  The caller supplies every buffer;
 * nothing is allocated, cleared or synchronised.
 *   form 0: C = [resid +] m c (A B^T + bias) [+ the old C when accum != 0]; act (or NULL) = gelu(C).  bias [N], resid and act
 *           [M, N] or NULL.  dropout (or NULL, or p == 0: none) puts the row site `site` (BT_DROP_ATTN_OUT, _FF_HIDDEN or _FF_OUT)
 *           over the [M, N] result, N a multiple of 4: drop_act == 0 masks the value before the residual as written above,
 *           drop_act != 0 leaves C alone and masks act = m c gelu(C) (act must be given)
 *   form 1: C (+)= A B; accum as above, the other optional arguments must be NULL
 *   form 2: C = A^T B over K summed rows the way a weight gradient is taken: one launch writes the partials of the
 *           BT_TRAIN_DW_ROWS-row chunks into ws ([chunks][M][N] floats, bt_train_matmul_workspace_bytes), a second adds them
 *           in chunk order; every optional argument must be NULL / 0
 * ws / ws_bytes: form 2 only (too small: BT_ERR_WORKSPACE); bt_train_matmul_workspace_bytes is 0 for the other forms. */
size_t bt_train_matmul_workspace_bytes(int form, int M, int N, int K);
int bt_train_matmul(void* stream, int mixed, int form, const float* A, const float* B, int M, int N, int K, float* C,
                    const float* bias, const float* resid, int accum, float* act, const bt_train_dropout* dropout_or_null,
                    int site, int drop_act, void* ws, size_t ws_bytes);
/* DIAGNOSTIC: the attention sweeps of either route on their own, launched as the unit calls launch them (blocks of
 * BT_TRAIN_ATTN_BLOCK queries on the fp32 route, of 32 on the mixed one).  qkv [B T, 3 dim] is what the sweeps read after RoPE:
 * q | k | v, head h in columns 32 h of each section; dim a multiple of 32 from 32 to 1024, B <= 65535, B T <= 2^22; qkv, O, dO
 * and dqkv 16-byte aligned.  dropout (or NULL, or p == 0: none) is the BT_DROP_ATTN_P site.  `mixed` as bt_train_matmul's: 0, 1
 * (fp16 operands), 2 (bfloat16 operands) or 4 (split bfloat16 operands), anything else is BT_ERR_ARG ahead of every other check.
 *   backward == 0: writes O [B T, dim] (before the gate; the dropped output with dropout) and lse [B T, dim / 32]
 *   backward != 0: reads dO [B T, dim], lse and delta [B T, dim / 32] (= sum_d dO O per row and head), runs the dK / dV sweep and
 *                  the dQ sweep and writes every element of dqkv [B T, 3 dim], the gradient before the backward RoPE
 * The arguments of the other direction may be NULL. */
int bt_train_attention(void* stream, int mixed, int backward, int B, int T, int dim, const float* qkv,
                       const bt_train_dropout* dropout_or_null, float* O, float* lse, const float* dO, const float* delta,
                       float* dqkv);

/* ---- training: the frontend's own units (csrc/train_front.hip) ------------------------------------------
 * What BeatThis.frontend holds beside its twelve attention / feed-forward leaves (those are BT_UNIT_ATTN / BT_UNIT_FF calls of
 * bt_train_forward / bt_train_backward on (B', T') = (B T, F) and (B F, T) rows).  Activations are this library's (b, t, f, c),
 * channels last, fp32 and contiguous; parameters are read in the REFERENCE's layout straight from the nn.Parameter storage and
 * gradients are written in that layout.  BatchNorm uses its RUNNING statistics (s = weight / sqrt(running_var + 1e-5), sh =
 * bias - running_mean s, evaluated in fp64 and rounded once); the statistics are never written and get no gradient.
 *   BT_FRONT_STEM    x [B, T, 128] -> y [B, T, 32, 32] = gelu(bn2d(conv(bn1d(x)))), F = 128, C = 32: w = stem.conv2d.weight
 *                    [32][1][4][3] (kernel (4, 3), stride (4, 1), padding (0, 1) over (f, t)), bn_* = stem.bn2d, bn1_* = stem.bn1d
 *   BT_FRONT_CONV    x [B, T, F, C] -> y [B, T, F / 2, 2 C] = gelu(s pre + sh), w = blocks.i.conv2d.weight [2 C][C][2][3]
 *                    (kernel (2, 3), stride (2, 1), padding (0, 1), no bias), bn_* = blocks.i.norm [2 C];
 *                    pre[b, t, f', co] = sum_{dt < 3, df < 2, ci} w[co][ci][df][dt] x[b, t + dt - 1, 2 f' + df, ci];
 *                    the forward also writes save_pre [B, T, F / 2, 2 C] = pre, which the backward reads.  F even, <= 32; C a
 *                    multiple of 32, <= 512.  The three matrix products run on v_mfma_f32_32x32x2_f32 as implicit GEMMs.
 *   BT_FRONT_LINEAR  x [B, T, F, C] -> y [B, T, dim] = frontend.linear of the reference's "b t (c f)" rows: w [dim][C F] with
 *                    column c F + f, b [dim]
 *   BT_FRONT_SWAP    x [B, T, F, C] -> y [B, F, T, C]; the backward takes gy [B, F, T, C] and writes gx [B, T, F, C].  T and F are
 *                    the two swapped extents, whichever holds the time: the way back is the same call with them exchanged; its
 *                    limits are B T F <= 2^22 rows and C <= 1024
 * The backward takes x (not BT_FRONT_SWAP), save_pre (BT_FRONT_CONV), the upstream gradient gy (shaped like y) and OVERWRITES the
 * gradients whose pointer is not NULL: gx (the stem's: the gradient of the spectrogram), g_w, g_b (projection), g_bn_w / g_bn_b
 * (bn2d, blocks.i.norm: sum of g_pre (pre - mean) / sqrt(var + eps) and of g_pre, g_pre = gy gelu'(s pre + sh)), g_bn1_w / g_bn1_b
 * (bn1d).  The contract is section 13's: no atomics; every gradient byte is written by one thread of one launch; the order of
 * every sum depends on the shapes alone (a GEMM element sums k ascending; weight gradients over chunks of BT_TRAIN_DW_ROWS rows,
 * column sums over chunks of BT_TRAIN_CS_ROWS rows, partials in the workspace added in chunk order by a second launch), so two
 * runs are bit-identical, and a sequence's gx is the same alone and inside a batch.  No call synchronises, allocates or clears
 * memory; no launch reads workspace bytes that the same call has not written.  Limits: B T <= 65535 (the frequency direction
 * runs one sequence per frame) and B T 32 <= 2^22 rows (BT_FRONT_SWAP: see above); anything else is BT_ERR_ARG and the workspace query returns 0.
 * These two entry points and the two bt_front_bn_* ones below check, before any launch and in this order, the struct pointer, the
 * shape, `mixed`, the required pointers, the workspace's alignment and its size; a call with several faults reports the first. */
#define BT_FRONT_STEM 0
#define BT_FRONT_CONV 1
#define BT_FRONT_LINEAR 2
#define BT_FRONT_SWAP 3
typedef struct {
  int32_t B, T, F, C, dim, mixed;
  int32_t operand;   /* read only when mixed == 1: BT_OPERAND_F16, _BF16 (section 24) or _BF16X3 (section 25) */
  int32_t reserved2;
  const float* w; const float* b;
  const float* bn_w; const float* bn_b; const float* bn_mean; const float* bn_var;
  const float* bn1_w; const float* bn1_b; const float* bn1_mean; const float* bn1_var;
  const float* x; float* y; float* save_pre;
  const float* gy;
  float* gx; float* g_w; float* g_b; float* g_bn_w; float* g_bn_b; float* g_bn1_w; float* g_bn1_b;
  void* ws; size_t ws_bytes;
} bt_front_args;
/* sizeof, then offsetof w, x, gy, gx, ws, ws_bytes: seven entries, the binding's self-check */
void bt_front_struct_sizes(int32_t* out);
size_t bt_front_workspace_bytes(int unit, int backward, int B, int T, int F, int C, int dim);
int bt_front_forward(void* stream, int unit, const bt_front_args* a);
int bt_front_backward(void* stream, int unit, const bt_front_args* a);

/* ---- training: the frontend's BatchNorm on BATCH statistics (csrc/train_front.hip) --------------------------
 * BT_FRONT_STEM and BT_FRONT_CONV as above, with torch's training-mode nn.BatchNorm1d / 2d (eps 1e-5, momentum 0.1, affine,
 * tracking) in place of the running statistics.  Over the n values of a channel (n = B T for bn1d, B T F' for bn2d and
 * blocks.i.norm, F' the output bins):
 *   forward   mean_b and the biased var_b of this call's batch: per chunk of BT_TRAIN_CS_ROWS rows the mean and the sum of
 *             squared deviations from it (fp64, rows ascending), merged in chunk order by a second launch (Chan's formula, fp64:
 *             one workgroup per channel, 256 runs of consecutive chunks and then the runs pairwise, left neighbour first -- a
 *             fixed tree over the shapes alone) and rounded once; y uses s = weight rstd_b, sh = bias - mean_b s with rstd_b = 1 / sqrt(var_b + 1e-5).  The same
 *             launch writes save_mean / save_rstd (save1_*: bn1d) and moves the running buffers IN PLACE, once per call:
 *             running_mean = 0.9 running_mean + 0.1 mean_b, running_var = 0.9 running_var + 0.1 var_b n / (n - 1) (fp64, rounded
 *             once), *tracked += 1 by one thread (a NULL tracked pointer: no count).  The stem takes the statistics of x first,
 *             stages pre = conv(bn1d(x)) in the workspace and takes bn2d's from it; the time padding stays zero AFTER bn1d.
 *             The conv unit writes save_pre as above.
 *   backward  reads x, w, the gains and biases, save_mean / save_rstd (and save_pre) -- never the running buffers, which it
 *             leaves alone.  With g the gradient at a BatchNorm's output and xhat = (v - mean_b) rstd_b: g_bias = sum g,
 *             g_weight = sum g xhat (always computed; into the workspace when the pointer is NULL), and the gradient at the
 *             BatchNorm's input is weight rstd_b (g - g_bias / n - xhat g_weight / n): the statistics are differentiated through.
 * So a sequence's gx is NOT the same alone and inside a batch, and the forward WRITES to the buffers it is handed.  The rest
 * of the contract is the one above: no atomics, one writer per output byte, summation orders from the shapes alone (two runs
 * from the same buffers are bit-identical), no synchronisation, allocation or clearing, no read of unwritten workspace.
 * n = 1 (torch: "Expected more than 1 value per channel when training") is BT_ERR_ARG before any launch, like every shape the
 * calls above refuse and every NULL among the required pointers; the workspace query then returns 0. */
typedef struct {
  int32_t B, T, F, C, mixed;
  int32_t operand;   /* read only when mixed == 1: BT_OPERAND_F16, _BF16 (section 24) or _BF16X3 (section 25) */
  int32_t reserved2, reserved3;
  const float* w;
  const float* bn_w; const float* bn_b; float* bn_mean; float* bn_var; int64_t* bn_tracked;
  const float* bn1_w; const float* bn1_b; float* bn1_mean; float* bn1_var; int64_t* bn1_tracked;
  float* save_mean; float* save_rstd; float* save1_mean; float* save1_rstd;
  const float* x; float* y; float* save_pre;
  const float* gy;
  float* gx; float* g_w; float* g_bn_w; float* g_bn_b; float* g_bn1_w; float* g_bn1_b;
  void* ws; size_t ws_bytes;
} bt_front_bn_args;
/* sizeof, then offsetof w, bn_tracked, save_mean, x, gy, gx, ws, ws_bytes: nine entries, the binding's self-check */
void bt_front_bn_struct_sizes(int32_t* out);
size_t bt_front_bn_workspace_bytes(int unit, int backward, int B, int T, int F, int C);
int bt_front_bn_forward(void* stream, int unit, const bt_front_bn_args* a);
int bt_front_bn_backward(void* stream, int unit, const bt_front_bn_args* a);

/* ---- training: 16-mixed in the frontend (csrc/train_front_mixed.inc) -------------------------------------
 * The `mixed` field of both argument structs above is their first reserved int32; the layouts and the self-checks are
 * unchanged.  0 selects the launches described above, bit for bit.  1 extends the 16-mixed contract of bt_train_forward_mixed
 * to the frontend's own products: BOTH operands of every matrix product are rounded to IEEE fp16 (to nearest even; beyond
 * fp16's range: inf) as they are staged, and the products accumulate in fp32 on v_mfma_f32_32x32x16_f16.
 *   BT_FRONT_CONV    pre = A W^T, g_x = G W and g_W = G^T A.  A is the implicit im2col of x: rows (b, t, f'), columns
 *                    dt 2 C + df C + ci, zero where frame t + dt - 1 lies outside the row's own sequence; G = g_pre s is multiplied
 *                    in fp32 and then rounded.  A small launch at the head of the call packs the weight once into an fp16 image
 *                    in the workspace ([co][dt][df C + ci] for the forward, its transpose for g_x): the same values, rounded
 *                    the same way.  The epilogues are the fp32 kernels': pre and gelu(s pre + sh), per-chunk partials of g_W.
 *   BT_FRONT_LINEAR  (bt_front_args only) forms 0, 1 and 2 of bt_train_matmul with mixed = 1.
 * With bt_front_bn_forward / _backward (BT_FRONT_CONV) the forward takes the moments of the fp16-product pre and the backward's
 * two GEMMs run mixed on the centred g_pre.  The frontend's twelve leaves are bt_train_forward_mixed / bt_train_backward_mixed
 * calls with residual = 1.  Everything else stays fp32 and stays the code above: the stem (K = 12: no product worth an MFMA),
 * BatchNorm folding, statistics and centring, GELU and its derivative, save_pre, the swaps, the column sums and the chunked g_W
 * reduction, parameters, saved tensors and gradients.  Nothing clamps: a loss scaler sees an overflow in the gradient norm.
 * Kept from section 13: no atomics; one writer per output byte; every order of summation depends on the shapes alone -- a
 * forward or backward-data element sums k ascending in MFMA steps of 16, g_W sums the rows ascending in steps of 16 inside each
 * chunk of BT_TRAIN_DW_ROWS rows and the chunks are added in order by the unchanged reduction -- so two runs are bit-identical;
 * on running statistics a sequence's g_x is the same alone and inside a batch; no call synchronises, allocates or clears
 * memory; no launch reads workspace bytes its own call has not written.
 * mixed = 1 with BT_FRONT_STEM or BT_FRONT_SWAP (or BT_FRONT_LINEAR in bt_front_bn_args), and any value other than 0 and 1, is
 * BT_ERR_ARG before any launch.  mixed = 1 needs a 16-byte aligned workspace of the size the two queries below return (the
 * fp32 size plus the weight image); they take the parameters of the fp32 queries, whose values are unchanged, and return 0 for
 * unsupported shapes and for units that have no mixed form.
 * `operand`, the int32 behind `mixed` in both structs (their former reserved1, same offsets), is read only
 * when mixed == 1 and checked together with it: BT_OPERAND_F16 is everything above; BT_OPERAND_BF16 rounds both operands of the
 * same products to bfloat16 (to nearest even, NaN stays NaN, nothing overflows by rounding) on v_mfma_f32_32x32x16_bf16, the
 * weight image holding bfloat16 in the same bytes, BT_FRONT_LINEAR calling bt_train_matmul with mixed = 2; any other value is
 * BT_ERR_ARG before any launch ("operand" in bt_last_error()).  With mixed == 0 the field is ignored.  The workspace queries do
 * not depend on it.
 * BT_OPERAND_BF16X3 (section 25) runs the same products on split bfloat16 operands, as described at the define: the packing
 * launch writes a hi and a lo weight image, activations and G are split while staged, BT_FRONT_LINEAR calls bt_train_matmul
 * with mixed = 4.  Because the image doubles, its workspace comes from the two *_x3 queries: the parameters of the fp32 queries,
 * the fp32 size plus both images, 0 for unsupported shapes and for units that have no mixed form.  A workspace smaller than that
 * is BT_ERR_WORKSPACE.  The *_mixed queries and their values are unchanged. */
size_t bt_front_workspace_bytes_mixed(int unit, int backward, int B, int T, int F, int C, int dim);
size_t bt_front_bn_workspace_bytes_mixed(int unit, int backward, int B, int T, int F, int C);
size_t bt_front_workspace_bytes_x3(int unit, int backward, int B, int T, int F, int C, int dim);
size_t bt_front_bn_workspace_bytes_x3(int unit, int backward, int B, int T, int F, int C);

/* ---- training: the optimiser step (csrc/optim.hip) ------------------------------------------------------
 * Multi-tensor AdamW with torch.optim.AdamW's default semantics (decoupled decay, no amsgrad, no maximize), all fp32.  With
 * gs = grad_scale (times *d_coef when d_coef is given, multiplied in fp32) every element does, one operation at a time and
 * without multiply-add contraction:
 *     g = grad * gs;   p = p * decay;   m = m + (g - m) * one_minus_beta1;   v = v * beta2 + (g * g) * one_minus_beta2;
 *     p = p - step_size * (m / (sqrt(v) / bias2_sqrt + eps))
 * where the caller computes, per group and in fp64 before rounding to fp32: decay = 1 - lr wd, step_size = lr / (1 - beta1^t),
 * bias2_sqrt = sqrt(1 - beta2^t).  Divide and square root are correctly rounded, denormals are kept: the device and the host
 * twin agree bit for bit.
 * Layout: gradients, m and v live in three flat fp32 buffers of `total` elements (16-byte aligned); tensor i occupies
 * [offset, offset + numel) of each, offset a multiple of 4, the padding between tensors is zero and never written.  The
 * parameters stay in their own storage (`param`, 4-byte aligned; 16-byte aligned ones are moved 16 bytes at a time).  One
 * workgroup of 256 threads updates one chunk of BT_OPTIM_CHUNK elements of one tensor: the chunk table lists (tensor, chunk
 * within the tensor) for every chunk.  bt_optim_plan, on the host, lays the tensors out and fills both tables: `tensors` must
 * hold n_tensors records; `chunks` may be NULL (sizing call) or hold chunk_capacity records; *total and *n_chunks are always
 * written.  zero_grads != 0: the pass stores 0 over every gradient it has consumed.
 * Global gradient norm: bt_grad_norm writes one fp64 sum of squares per slice of BT_OPTIM_NORM_SLICE elements of the flat
 * gradient buffer into the workspace (launch 1; 256 threads, each its elements in ascending order, then a 256-leaf tree) and
 * adds them in index order (launch 2, one workgroup); record[0] = norm = sqrt(sum) |grad_scale| and record[1] = coef =
 * min(1, max_norm / (norm + 1e-6)) as fp32 (torch.nn.utils.clip_grad_norm_; a non-finite norm propagates as in torch).
 * No call synchronises, allocates, clears memory or uses atomics; the order of every sum depends on the layout alone. */
#define BT_OPTIM_CHUNK 4096
#define BT_OPTIM_NORM_SLICE 4096
#define BT_OPTIM_MAX_GROUPS 8
typedef struct {
  float* param; int64_t offset, numel; int32_t group, reserved;
} bt_optim_tensor;
typedef struct {
  int32_t tensor, chunk;
} bt_optim_chunk;
typedef struct {
  float decay, one_minus_beta1, beta2, one_minus_beta2, step_size, bias2_sqrt, eps, reserved;
} bt_optim_group;
typedef struct {
  int32_t n_groups, zero_grads; float grad_scale; int32_t reserved;
  bt_optim_group g[BT_OPTIM_MAX_GROUPS];
} bt_optim_hyper;
/* sizeof of the four structs, offsetof offset and group (tensor record) and g (hyper), then BT_OPTIM_CHUNK, BT_OPTIM_NORM_SLICE
 * and BT_OPTIM_MAX_GROUPS: ten entries, the binding's self-check */
void bt_optim_struct_sizes(int32_t* out);
/* HOST */
int bt_optim_plan(int n_tensors, const void* const* params, const int64_t* numel, const int32_t* groups, int n_groups,
                  bt_optim_tensor* tensors, int64_t* total, bt_optim_chunk* chunks, int64_t chunk_capacity, int64_t* n_chunks);
size_t bt_grad_norm_workspace_bytes(int64_t total);
int bt_grad_norm(void* stream, const float* d_grad, int64_t total, float grad_scale, float max_norm, void* d_ws, size_t ws_bytes,
                 float* d_record);
int bt_adamw_step(void* stream, const bt_optim_tensor* d_tensors, int n_tensors, const bt_optim_chunk* d_chunks, int64_t n_chunks,
                  float* d_grad, float* d_m, float* d_v, int64_t total, const bt_optim_hyper* hyper, const float* d_coef);
/* HOST: the same arithmetic in the same order on host arrays (`param` of the tensor records: host pointers); the tables are
 * validated entry by entry */
int bt_grad_norm_host(const float* grad, int64_t total, float grad_scale, float max_norm, float* record);
int bt_adamw_step_host(const bt_optim_tensor* tensors, int n_tensors, const bt_optim_chunk* chunks, int64_t n_chunks, float* grad,
                       float* m, float* v, int64_t total, const bt_optim_hyper* hyper, const float* coef);
/* Weight averaging: the exponential moving average of the parameters that
 * torch.optim.swa_utils.AveragedModel keeps with get_ema_multi_avg_fn(decay), made in the pass of the step.  The AdamW step
 * above with a fourth flat fp32 buffer d_ema, laid out, aligned and refused like m and v.  The thread that updates an element
 * first computes its new p exactly as the plain step does (p, m, v and the cleared gradient have the plain step's bits) and
 * THEN moves the element's average e from that new p:
 *     ema_copy != 0:   e = p                        (the first averaged step; the old e is not read)
 *     ema_copy == 0:   e = e + (p - e) * ema_weight   (a subtraction, a product, a sum: each rounded to fp32 once, no contraction)
 * ema_weight = 1 - decay, computed by the caller in fp64 and rounded to fp32 once; a value that is not a number in (0, 1] is
 * BT_ERR_ARG before any launch, whatever ema_copy is.  Only a chunk's owner writes its part of d_ema, the padding between
 * tensors is never written, a damaged table updates nothing; no atomics, memsets or allocation.
 * The limit of every fp32 average: once |(p - e) * ema_weight| is below half an ulp of e, e stops moving.  With decay 0.9999
 * and parameter steps of 1e-5, torch's own fp32 EMA is then about 1e-2 (relative to the displacement of the average) from
 * an fp64 one; this arithmetic is within a few percent of torch's.  Documented, not repaired.
 * The exchange swaps p and e element by element over the same tables (16 bytes at a time, one element at a time for a
 * 4-byte aligned parameter and the tail): a pure move, twice is the identity. */
int bt_adamw_ema_step(void* stream, const bt_optim_tensor* d_tensors, int n_tensors, const bt_optim_chunk* d_chunks,
                      int64_t n_chunks, float* d_grad, float* d_m, float* d_v, float* d_ema, int64_t total,
                      const bt_optim_hyper* hyper, const float* d_coef, float ema_weight, int ema_copy);
int bt_ema_exchange(void* stream, const bt_optim_tensor* d_tensors, int n_tensors, const bt_optim_chunk* d_chunks, int64_t n_chunks,
                    float* d_ema, int64_t total);
/* HOST: the twin of the averaging step, bit-identical to the device */
int bt_adamw_ema_step_host(const bt_optim_tensor* tensors, int n_tensors, const bt_optim_chunk* chunks, int64_t n_chunks,
                           float* grad, float* m, float* v, float* ema, int64_t total, const bt_optim_hyper* hyper,
                           const float* coef, float ema_weight, int ema_copy);

/* ---- building bundles from audio: time stretch, pitch shift, arbitrary-ratio resampling (csrc/stretch.hip, DESIGN.md
 * section 20) -------------------------------------------------------------------------------------------------------------------
 * The reference's launch_scripts/preprocess_audio.py makes its tempo and pitch variants with pedalboard (Rubber Band).  That
 * algorithm cannot be restated; the one below is this library's own and THIS TEXT is its definition (tests/stretch_reference.py
 * is a numpy restatement of it).  What is kept of the reference is the meaning of its parameters: a tempo change of +p percent
 * shortens the audio to 1 / (1 + p / 100) of its length, a pitch shift of s semitones keeps the length.
 *
 * TIME STRETCH  x[0 .. N) fp32 (zero outside), length factor L, 0.5 <= L <= 2  ->  y[0 .. M), M = floor(N L + 0.5) (fp64).
 * Phase vocoder with identity phase locking (Laroche & Dolson 1999, the basic form).  n_fft = 2048, periodic Hann window
 * w[i] = 0.5 - 0.5 cos(2 pi i / 2048) for analysis and synthesis, synthesis hop Hs = 512, real FFT, bins k = 0 .. 1024.  A frame
 * "centred at c" is x[c - 1024 + i] w[i], i = 0 .. 2047, and X[k] = sum_i of it times exp(-2 pi i k i / 2048).
 *   Frames: n = 0 .. ceil(M / Hs), frame n centred at OUTPUT sample n Hs.  It takes two analysis frames: X1_n centred at
 *     a_n = floor(n Hs / L + 0.5) (fp64) and X0_n centred at a_n - Hs.
 *   Phases are 32-bit fixed-point turns: q(z) = round(atan2(im, re) / (2 pi) * 2^32) mod 2^32, round to nearest, q(0) = 0.  The two
 *     analysis frames are one synthesis hop apart, so the unwrapped phase advance of the classical vocoder is congruent to
 *     d[n,k] = q(X1_n[k]) - q(X0_n[k]) (uint32; d[0,k] = q(X1_0[k])) and the accumulated phase is the integer prefix sum
 *     S[n,k] = sum_{m = 0 .. n} d[m,k] (uint32): exact, independent of the order of summation.
 *   Locking, per frame on mag = |X1_n|: bin k is a PEAK iff mag[k] > 0, mag[k] > mag[j] for the existing j of {k - 2, k - 1} and
 *     mag[k] >= mag[j] for the existing j of {k + 1, k + 2}.  A bin b between consecutive peaks p < p' belongs to p iff
 *     b <= (p + p') / 2 (integer division), bins below the first peak to the first, bins above the last to the last; in a
 *     frame without a peak every bin belongs to itself.  With p(k) the owner of k:
 *     phi[n,k] = S[n,p(k)] + q(X1_n[k]) - q(X1_n[p(k)])  (uint32).
 *   Synthesis: Y_n[k] = mag[k] exp(2 pi i phi[n,k] / 2^32), imaginary parts of bins 0 and 1024 dropped; y_n = inverse real FFT
 *     (1 / 2048 normalised) times w.  Output sample m = sum over its at most four frames (those with 0 <= m - n Hs + 1024 < 2048),
 *     in ascending n, of y_n[m - n Hs + 1024], divided by the sum of w^2 at the same indices over the same frames.
 *   At L = 1, X0_n = X1_{n-1}: the sum telescopes, phi = q(X1_n) whatever the peaks are, and y = x up to rounding.
 * Arithmetic: the analysis (FFT, magnitude, atan2) is fp64 -- which bin is a peak is decided as the definition decides it, not by
 * fp32 rounding -- and the synthesis fp32.  No atomics: two calls give the same bits.
 * Limits: 1 <= N, M <= BT_STRETCH_MAX_SAMPLES (25 minutes at 44.1 kHz).  The workspace is the caller's, 16-byte aligned,
 * bt_stretch_workspace_bytes (N, L) bytes (0: unsupported N or L; about 20.6 KB per 512 output samples); no launch reads a byte
 * of it that this call has not written.  bt_stretch_out_len (N, L) = M (0: unsupported); n_out must equal it.
 * d_tables: BT_STRETCH_TABLE_DOUBLES doubles -- w[2048], then (cos, -sin)(2 pi t / 1024) for t = 0 .. 1023, then
 * (cos, -sin)(2 pi k / 2048) for k = 0 .. 1024 (beat_this_amd/tables.py: stretch_tables).
 * The prefix sum runs in blocks of BT_STRETCH_SCAN_BLOCK frames (tests sit on both sides of the boundary).
 *
 * RESAMPLING BY AN ARBITRARY RATIO  y[m] = c sum_j x[j] h(c (m step - j)), m = 0 .. n_out - 1, c = min(1, 1 / step), x zero outside
 * [0, n_in); 0.25 <= step <= 4, 1 <= n_in, n_out <= 4 BT_STRETCH_MAX_SAMPLES.  h(t) = 2 fc sinc(2 fc t) kaiser(t / Z), fc = 0.47825, |t| < Z = BT_RESAMPLE_RATIO_CROSSINGS, is read
 * from d_table = h(i / P), i = 0 .. P Z, P = BT_RESAMPLE_RATIO_TAPS (fp32, tables.py: resample_ratio_table) by linear
 * interpolation: u = |c (m step - j)| P in fp64, i = floor(u), h = tab[i] + (u - i)(tab[i+1] - tab[i]) in fp32.  The position
 * m step and u are fp64 (fp32 positions are wrong after a few seconds of audio); products and the sum are fp32, taps in ascending j
 * from ceil(m step - Z / c), floor(2 Z / c) + 1 of them.
 * PITCH SHIFT by s semitones = bt_stretch with L = r = 2^(s / 12), then bt_resample_ratio with step = r to exactly N samples. */
#define BT_STRETCH_MAX_SAMPLES (1 << 26)
#define BT_STRETCH_SCAN_BLOCK 64
#define BT_STRETCH_TABLE_DOUBLES 6146
#define BT_RESAMPLE_RATIO_TAPS 4096
#define BT_RESAMPLE_RATIO_CROSSINGS 116
int64_t bt_stretch_out_len(int64_t n_in, double L);
size_t bt_stretch_workspace_bytes(int64_t n_in, double L);
int bt_stretch(void* stream, const double* d_tables, const float* d_in, int64_t n_in, double L, float* d_out, int64_t n_out,
               void* d_ws, size_t ws_bytes);
int bt_resample_ratio(void* stream, const float* d_in, int64_t n_in, double step, const float* d_table, float* d_out,
                      int64_t n_out);

/* ---- PCM decode (csrc/pcm.hip): the `data` chunk of a little-endian RIFF/WAVE file -> the mono fp32 waveform, on the device.
 * Input: interleaved frames of C channels in one of six sample formats; every sample has an exact real value s:
 *   BT_PCM_U8   s = (v - 128) / 128          BT_PCM_S32  s = v / 2^31
 *   BT_PCM_S16  s = v / 2^15                 BT_PCM_F32  s = the sample
 *   BT_PCM_S24  s = v / 2^23 (3 bytes)       BT_PCM_F64  s = the sample
 * all exact in fp64.
 *   C = 1: out = fp32(s), round to nearest even (an f32 sample is copied as it is; -0 stays -0).
 *   C > 1: acc = (+0.0) + s[0]; acc = acc + s[c] for c = 1 .. C-1 in that order; acc = acc / C (IEEE division); out =
 *          fp32(acc); all in fp64.  This is numpy's `signal.mean(1)` of the float64 (frames, C) array followed by the fp32
 *          conversion (preprocessing.load_audio through scipy or soundfile, Audio2Frames.signal2spect): numpy (2.2) starts the
 *          row sum at +0.0 and adds the contiguous channel axis left to right up to 7 channels, in an unrolled order from 8 on.
 *          The leading +0.0 only matters for the sign of zero: a frame of -0.0 in every channel gives +0.0 where C > 1.
 * Channels: 1 .. BT_PCM_MAX_CHANNELS_INT for the integer formats (their sums are exact in any order), 1 ..
 * BT_PCM_MAX_CHANNELS_FLOAT for f32 / f64.  No multiply-add contraction changes a result (the source is built with
 * -ffp-contract=off), results that are fp32 subnormals keep gradual underflow, NaN stays NaN (its payload and sign are not
 * part of the contract).
 * Pointers: d_src may have ANY byte alignment (the data chunk of a real file starts 44, 46, 58, 68 ... bytes into the upload).
 * The kernel reads only inside the aligned 16-byte windows that enclose [d_src, d_src + n_frames C bytes_per_sample); the caller
 * guarantees that those windows lie inside its allocation; no result depends on a byte outside the payload.  d_out is 16-byte
 * aligned; exactly n_frames floats are written.  A track of 0 frames is legal and writes nothing.  No atomics, no workspace:
 * runs are bit-identical.  BT_ERR_ARG, before any launch: a null pointer, an unknown format, a channel count outside the
 * contract, a negative count, more than BT_PCM_MAX_TRACKS tracks. */
#define BT_PCM_U8 0
#define BT_PCM_S16 1
#define BT_PCM_S24 2
#define BT_PCM_S32 3
#define BT_PCM_F32 4
#define BT_PCM_F64 5
#define BT_PCM_MAX_CHANNELS_INT 8
#define BT_PCM_MAX_CHANNELS_FLOAT 7
#define BT_PCM_MAX_TRACKS 65535
#define BT_PCM_THREAD_FRAMES 4      /* frames per thread: one 16-byte store */
#define BT_PCM_BLOCK_FRAMES 1024    /* frames per workgroup */
typedef struct { const uint8_t* d_src; int64_t n_frames; float* d_out; int32_t format; int32_t channels; } bt_pcm_span;
/* one launch for a ragged list of tracks (a DEVICE table; formats may differ between tracks); max_frames = the largest n_frames.
 * The table's entries are checked by the caller: the launch trusts them (the host cannot read a device table without a copy). */
int bt_pcm_decode_batch(void* stream, const bt_pcm_span* d_tracks, int n_tracks, int64_t max_frames);
/* one track without a device table (the single-file latency path) */
int bt_pcm_decode(void* stream, const uint8_t* d_src, int format, int channels, int64_t n_frames, float* d_out);
/* the host twin: plain sequential C++ over the same inline helpers; src and out in HOST memory, any alignment of src */
int bt_pcm_decode_host(const uint8_t* src, int format, int channels, int64_t n_frames, float* out);

/* ---- FLAC decode (csrc/flac.hip, csrc/flac_bits.h): a FLAC file's bytes -> the mono fp32 waveform, on
 * the device, frame search included.  The format facts are RFC 9639's.
 * Accepted: native FLAC (the `fLaC` marker), optionally behind an ID3v2 tag; any metadata blocks before the audio (skipped by
 * their lengths; STREAMINFO first); 1 .. 8 channels; 4 .. 24 bits per sample; any block size up to 65535; fixed and variable
 * blocking; total_samples > 0; bytes behind the last frame are ignored.  Declined (the probe returns 0): Ogg FLAC,
 * total_samples == 0, 25 .. 32 bits per sample.  The device entry points also refuse (BT_ERR_ARG) a file of 2^31 bytes or
 * more and a stream of 2^31 samples or more.
 * Arithmetic: the decoded integers v are exact; a sample's value is s = v / 2^(bps-1), exact in fp64 (what soundfile and
 * torchaudio hand to load_audio).  One channel: out = fp32(s).  C channels: acc = (+0.0) + s[0]; acc = acc + s[c] left to
 * right; acc = acc / C; all in fp64, then one rounding to fp32 -- BT_PCM_S16 / BT_PCM_S24's words above, so a FLAC file and a
 * WAV file that hold the same integers decode to the same bits.  Integer sums of up to 8 channels are exact in any order.
 * The source is built with -ffp-contract=off.
 * Frames: a FLAC frame has no length field.  A frame is accepted only as a link of the chain that starts at first_frame: it
 * begins where the previous frame ended, its header is one of this stream (sync, the stream's blocking bit, no reserved
 * code, channels / sample size / rate as STREAMINFO has them, block size <= max_block, a well-formed coded number, CRC-8),
 * it carries the number that follows its predecessor's (frame index, or running sample count), its subframes, zero padding
 * and CRC-16 hold, and it does not pass total_samples.  The chain must end exactly at total_samples.  Checksums alone accept
 * nothing: a verbatim subframe may hold a complete valid frame as payload.  Anything else sets the track's status and writes
 * no output sample.
 * Status, per track: code BT_FLAC_OK, or BT_FLAC_BROKEN (no valid frame with the expected number at byte `where`),
 * BT_FLAC_LENGTH (the frame at `where` would pass total_samples), BT_FLAC_CANDIDATES (device only: more frame-header
 * candidates than the workspace provides for, n / 8 + 64 of them -- a valid stream without false headers cannot have more:
 * a frame has at least 9 bytes); n_frames / n_samples: what the chain had accepted; `where`: the byte at which the chain
 * broke, or the byte behind the last frame.
 * Device: a call decodes a ragged list of tracks in a number of launches that does not depend on the list (scan, prefix,
 * compact, measure, link, decode, mix; blockIdx.y = track).  No read leaves a track's [d_src, d_src + n_bytes); d_src may
 * have any alignment.  Writes: exactly total_samples floats at d_out (16-byte aligned) where the status is BT_FLAC_OK, none
 * otherwise; the status; and bytes of [d_ws, d_ws + the workspace query) (d_ws 16-byte aligned).  A workspace smaller than the
 * query is BT_ERR_WORKSPACE before any launch.  No atomics: output and status are bit-identical between runs, and between a
 * track alone and the same track in a batch.  The device and the host twin agree bit for bit in output and status. */
#define BT_FLAC_OK 0
#define BT_FLAC_BROKEN 1
#define BT_FLAC_LENGTH 2
#define BT_FLAC_CANDIDATES 3
#define BT_FLAC_MAX_TRACKS 65535
#define BT_FLAC_THREAD_SAMPLES 4     /* output samples per thread of the mix: one 16-byte store */
#define BT_FLAC_BLOCK_SAMPLES 1024   /* output samples per workgroup of the mix */
#define BT_FLAC_SCAN_BYTES 256       /* byte offsets per workgroup of the scan */
typedef struct {
  int32_t sample_rate, channels, bps, blocking;   /* blocking: the blocking bit of the first frame */
  int32_t min_block, max_block;
  int64_t total_samples, first_frame, n_bytes;    /* first_frame: byte offset of the first frame; n_bytes: the file's length */
  uint8_t md5[16];                                /* of the interleaved little-endian PCM (STREAMINFO) */
} bt_flac_info;
typedef struct { int32_t code; int32_t n_frames; int64_t n_samples; int64_t where; } bt_flac_status;
typedef struct { const uint8_t* d_src; float* d_out; void* d_ws; size_t ws_bytes; bt_flac_status* d_status; bt_flac_info info; } bt_flac_span;
/* HOST: marker, ID3v2 skip, metadata walk, STREAMINFO, the first frame's offset and blocking bit -> 1, or 0 for a file
 * outside the subset (or a null argument) */
int bt_flac_probe_host(const uint8_t* bytes, int64_t n_bytes, bt_flac_info* info);
/* HOST: the sequential twin over the same parser: out_f32 gets total_samples floats and pcm_i32_or_null (if given) the
 * total_samples x channels interleaved integers -- both only where the status is BT_FLAC_OK.  BT_ERR_ARG: a null argument,
 * an info outside the subset. */
int bt_flac_decode_host(const uint8_t* src, const bt_flac_info* info, float* out_f32, int32_t* pcm_i32_or_null,
                        bt_flac_status* status);
/* device workspace of one track (0 for an info outside the subset) */
size_t bt_flac_workspace_bytes(const bt_flac_info* info);
/* one call for a ragged list of tracks: h_tracks (HOST, read before the launches: sizes and checks) and d_tracks (DEVICE,
 * the same n_tracks entries: what the kernels read) */
int bt_flac_decode_batch(void* stream, const bt_flac_span* h_tracks, const bt_flac_span* d_tracks, int n_tracks);
/* one track without a device table */
int bt_flac_decode(void* stream, const uint8_t* d_src, const bt_flac_info* info, float* d_out, void* d_ws, size_t ws_bytes,
                   bt_flac_status* d_status);

/* ---- data-parallel training: the rank-ordered gradient sum (csrc/reduce.hip) ----------------------------
 * `world` fp32 arrays of n elements, rank r's at d_parts + r * stride (elements), are added element by element in RANK ORDER,
 * one rounded fp32 add at a time and nothing else:
 *     out[i] = (((parts[0 * stride + i] + parts[1 * stride + i]) + parts[2 * stride + i]) + ...) + parts[(world - 1) * stride + i]
 * for i = 0 .. n - 1.  That is the chain autograd's in-place accumulation forms over the same gradients in the same order, so
 * a sum over ranks has the bits of an accumulation over batches.  NaN and +-inf propagate as IEEE addition propagates them;
 * denormals are kept; world == 1 copies.  The device and the host twin agree bit for bit.
 * d_out may be exactly d_parts (rank 0's part is overwritten in place); any other overlap of [d_out, d_out + n) with the parts is
 * BT_ERR_ARG.  Also BT_ERR_ARG, before any launch: world outside 1 .. BT_REDUCE_MAX_WORLD, n < 0, stride < n with world > 1, a
 * null or not 4-byte aligned pointer.  n == 0 launches nothing.
 * One workgroup of 256 threads sums one chunk of BT_REDUCE_CHUNK elements; 16 bytes per access when d_parts and d_out are
 * 16-byte aligned and stride is a multiple of 4 (or world == 1), one element per lane otherwise and for the tail n % 4.  Only
 * out[0 .. n) is written; the parts are only read.  No workspace, no atomics, no synchronisation. */
#define BT_REDUCE_MAX_WORLD 16
#define BT_REDUCE_CHUNK 4096
int bt_grad_rank_sum(void* stream, const float* d_parts, int64_t stride, int world, int64_t n, float* d_out);
/* HOST: the same adds in the same order on host arrays */
int bt_grad_rank_sum_host(const float* parts, int64_t stride, int world, int64_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif
