// f5_kernels.h — launchers of the non-GEMM F5 kernels (f5_kernels.hip, attention.hip).
#pragma once
#include "common.h"

namespace mi {

enum { NORM_LN_MOD = 0, NORM_LN_AFFINE = 1, NORM_L2 = 2 };
// x fp32 [rows][D] -> y (out_dtype) ; LN_MOD: LN(x)*(1+a)+b ; LN_AFFINE: LN(x)*a+b ; L2: a*x/||x||+b
void launch_rownorm(int mode, const float* x, void* y, int out_dtype, const float* a, const float* b, long rows, int D,
                    float eps, hipStream_t s);
// ragged batches: items x Fmax rows out; row t of item i normalises x row offs[i] + t, rows t >= lens[i] are zeros (device tables)
void launch_rownorm_len(int mode, const float* x, void* y, int out_dtype, const float* a, const float* b, int items, int Fmax, int D,
                        float eps, const int* lens, const long* offs, hipStream_t s);
// LN_MOD with the result as gemm_x3p.hip panel planes (three-way bf16 split of the fp32 value) instead of fp32 rows
void launch_rownorm_x3p(const float* x, void* planes, const float* a, const float* b, long rows, int D, float eps, hipStream_t s,
                        int np = 3, int* sat = nullptr);       // sat: range watch of the fp16-pair split (x3_split.h)
// AdaLN fold (ConvGemm::ln_*, gemm_epilogue.h): the producer side as a pass of its own, for the first block of an evaluation —
// aout = x o (1 + scale) as panel planes of np planes (a_dtype MI_F32) or rows of a_dtype, stats[row][D / 32][2] = partial (sum, sum^2)
void launch_ln_prologue(const float* x, void* aout, int a_dtype, int np, float* stats, const float* scale, long rows, int D, int* sat,
                        hipStream_t s);
// ... and, for the 16-bit engines, the partials of every row summed once into fin[row] = (rstd, mean * rstd) (ConvGemm::ln_final)
void launch_ln_finalize(const float* partials, float* fin, long rows, int D, float eps, hipStream_t s);
void launch_ln_gather(const float* mod, long mod_ld, long col_scale, long col_shift, float* G, float* S, int steps, int D, hipStream_t s);
void launch_cast_to_f32(const void* src, int dtype, float* dst, long n, hipStream_t s);
void launch_absmax(const float* x, long n, unsigned* out_bits, hipStream_t s);       // atomicMax of the bit pattern of max |x|
void launch_dwconv7(const float* x, float* y, const float* w, const float* bias, int B, int T, int C, hipStream_t s);
void launch_grn(float* y, float* ss_scratch, const float* gamma, const float* beta, int B, int T, int C, hipStream_t s);
// ids [U][N]; out slabs 2u (text) / 2u+1 (drop)
void launch_text_gather(const int* ids, const float* emb, const float* pos, float* out, int U, int N, int C, hipStream_t s);
void launch_text_ids(const int32_t* in, int* out, int U, int T, int N, int vocab, int* err, hipStream_t s);
void launch_mask_rows(const int* ids, float* x, int V, int N, int C, hipStream_t s);
void launch_copy2d(const float* src, long lds_, void* dst, long ldd, long rows, int cols, int out_dtype, hipStream_t s);
void launch_pad_reflect(const int16_t* a, float* out, int U, long L, int half, hipStream_t s);
void launch_spec_mag(const float* spec, float* mag, int F, int nb, int ldm, float eps, hipStream_t s);      // sqrt(re^2 + im^2 + eps)
void launch_logmel(const float* melraw, float* cmt, float* cmtd, int U, int N, int R, int M, int ld, hipStream_t s);
void launch_vocos_head(const float* sp, float* c, long rows, int nb, int ldc, hipStream_t s);
void launch_istft_ola(const float* frames, const float* wsi, int U, int F, int nfft, int hop, float* out_f,
                      int16_t* out_i, hipStream_t s);
void launch_cat_noise(const float* noise, void* cat, int U, int N, int M, int ldc, int dtype, hipStream_t s);
void launch_cfg_update(float* noise, const float* pred, int U, int N, int M, float cfg, const float* dt, int k, hipStream_t s, int parts = 1);
// ragged batches (padded slabs of N rows, utterance u live in rows [0, len[u])): the same update, 0 in rows >= len[u]
void launch_cfg_update_len(float* noise, const float* pred, int U, int N, int M, float cfg, const float* dt, int k, const int* len,
                           hipStream_t s, int parts = 1);
// x [items][N][row_bytes]: rows >= len[item / per] set to zero (16-byte stores; row_bytes % 16 == 0)
void launch_zero_pad_rows(void* x, long row_bytes, int items, int N, const int* len, int per, hipStream_t s);
void launch_sum_parts(const float* in, float* out, long rows, int M, int parts, hipStream_t s);

// attention.hip: softmax_fp32(q k^T) v, no mask, no scale (q/k are pre-scaled): modules.py:467
//   q [BH][N][64], k, v in the layout of AttnKvLayout -> o [B][N][H*64] (dtype), B = BH / H
// One AttnPlan, made by attention_plan() BEFORE the QKV projection of an evaluation, decides both sides of the K / V contract: the
// layout the QKV epilogue writes (ConvGemm::kv_planes / k_ld / v_ld / v_rows are copied from plan.kv) and the kernel that reads it.
// The options and the engine's arithmetic (ArithScope) are read there and nowhere else.
struct AttnKvLayout {
    int kv_planes = 0;     // 0: k as rows [BH][N][64] of the engine's type.  2 | 3 (fp32 engines, both products split, a caller that can
                           // pre-split): k [BH][np][k_ld][64] as np = 2 fp16 {hi, lo} or 3 bf16 planes (x3_split.h), v alike: [BH][np][64][v_ld],
                           // or [BH][np][k_ld][64] with v_rows; the pad keys may hold any bytes, the kernel clears them
    long k_ld = 0;         // with kv_planes: N rounded up to the 64-key stage
    long v_ld = 0;         // 0: v as rows [BH][N][64] (fp32, native and q.k-split kernels); else v transposed [BH][64][v_ld]: N rounded up to 8
                           // (16-bit engines, and fp32 with both products split), to 64 with kv_planes
    int v_rows = 0;        // with kv_planes: v as rows like k (the kernel's VROWS form transposes on its LDS reads)
};
AttnKvLayout attention_kv_layout(int N, int dtype, bool caller_can_presplit_kv);
// the kernels: even = 128-query workgroups, + 1 = 64-query workgroups whose wave pairs share the keys (SPLIT2)
enum AttnForm {
    ATTN_F32 = 0, ATTN_F32_QK_X3 = 2, ATTN_X3F = 4, ATTN_X3F_BF16X3 = 6, ATTN_X3F_PAIRS = 8,      // fp32: native | q.k split | both split: K / V split in the kernel | pre-split, 3 bf16 planes | 2 fp16 planes
    ATTN_X3F_PAIRS_SLICED = 10,                                                                   // ... 128-query workgroups over (uneven) key slices
    ATTN_F16 = 11, ATTN_F16_REF = 13, ATTN_BF16 = 15, ATTN_FORMS = 17
};
// queries per workgroup, keys per LDS stage, and the key-slice workspace: one slot of partial (m, l, O) per (query tile, slice) — two
// 32-query groups per 64-query tile, four per 128-query tile — and one zeroed ticket counter per tile.  F5::ensure_workspace reserves
// ATTN_WS_TILES 64-query tiles x ATTN_MAX_SLICES; attention_plan() slices only what fits the workspace it is told of.
constexpr int ATTN_TILE = 128, ATTN_TILE_SPLIT = 64, ATTN_STAGE = 64, ATTN_MAX_SLICES = 4;
constexpr long ATTN_SLOT_GROUP = 32 * 64 + 64 * 2, ATTN_SLOT_SPLIT = 2 * ATTN_SLOT_GROUP, ATTN_SLOT = 4 * ATTN_SLOT_GROUP;      // floats
constexpr long ATTN_WS_TILES = 2048;
struct AttnPlan {
    AttnKvLayout kv;            // what the QKV epilogue must write
    bool o_planes = false;      // the kernel can also leave its output as gemm_x3p.hip panel planes of the [B * N][H * 64] matrix
    int form = ATTN_F32;        // AttnForm (+ 1: SPLIT2)
    bool varlen = false;        // ragged batch: launch_attention() is given the device table of lengths
    int BH = 0, H = 0, N = 0, dtype = MI_F32;
    unsigned grid[3] = {1, 1, 1};      // query tiles x BH x key slices
    int cut[3] = {0, 0, 0};     // ATTN_X3F_PAIRS_SLICED: cut[0] > 0 = uneven slices [0, cut[0]), [cut[0], cut[1]), ... in stages, longest first
    int xmap = 0;               // XCD-aware workgroup map (ATTN_XCD_MAP)
    float sscale = 1.f;         // ATTN_F16_REF: the reference's fp16 score form, scores rounded to fp16 and x sscale in fp32 (F5/fp16/modules.py:467)
    const char* label = "";     // the profiler's name of the launch (rocprofv3 shows the instantiation itself)
};
// ref_fp16_scale (f16 engines; 0 = off) selects ATTN_F16_REF.  ws_floats / cnt_n: the caller's key-slice workspace (0: none, every
// query tile is one workgroup).  has_lens: a ragged batch — the grid, the slices and the cuts are those of the uniform launch at N.
AttnPlan attention_plan(int BH, int H, int N, int dtype, bool caller_can_presplit_kv, bool has_lens, float ref_fp16_scale, long ws_floats,
                        long cnt_n);
// o_planes (null: rows in o) needs plan.o_planes; o_np = its planes per value (2 | 3).  ws / cnt: the workspace the plan was told of.
void launch_attention(const AttnPlan& plan, const void* q, const void* k, const void* v, void* o, void* o_planes, int o_np, float* ws,
                      int* cnt, const int* lens, hipStream_t s);

}  // namespace mi
