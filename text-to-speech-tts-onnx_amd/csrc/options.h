// options.h — every process-wide tuning option and every environment switch of the library: one table (MI_OPTIONS), one row each.
// Precedence, the same for every row: the default, then the environment (read ONCE for the whole table, by options_init() at the
// process's first C-ABI call — capi.hip guard() — so before any launch, any engine constructor and any mi_set_option), then
// mi_set_option.  Launch paths read a row by its enum index: opt(OPT_GEMM_SK) is one relaxed atomic load.
// Not read once, but through env_int / env_first_is below, so that every getenv and every parsing convention lives in options.hip:
// constructor-time switches, per-handle state (MI355TTS_NO_GRAPH, _CAT_PAD, _PROJ_PARTS, _NO_FUSED_AA, _FUSED_MAX_C), and switches
// read at the call (MI355TTS_GEMM_DBG, _AACONV_DBG; _BENCH_ZERO / _BENCH_WSETS inside mi_bench_conv_gemm).
// The per-engine arithmetic override (ArithOverride / ArithScope, common.h) is a thread-local layer OVER this table, not part of it.
#pragma once
#include <atomic>
#include <shared_mutex>

namespace mi {

// How a row's environment variable maps to a value.
//   ENV_INT      the integer as given, then the row's policy (clamped; != 0 for a BOOL row; outside a REJECT row's range: default)
//   ENV_ONE_OFF  first character '1' -> 0, anything else keeps the default (the MI355TTS_NO_* names)
//   ENV_ZERO_OFF first character '0' -> 0, anything else keeps the default
//   ENV_ONE_ON   first character '1' -> 1, anything else keeps the default
//   ENV_CUTS     MI355TTS_ATTN_CUTS: "7,14" -> up to three cut points (opt_attn_cuts()); the row holds how many were given
// What mi_set_option does with a value.
//   STORE as given | BOOL v != 0 | CLAMP into [lo, hi] | REJECT: outside [lo, hi] the call fails and the value stays
//
//   X(enum suffix, mi_set_option key or nullptr, environment variable or nullptr, env convention, default, policy, lo, hi)
#define MI_OPTIONS(X)                                                                                                   \
    /* implicit-GEMM launcher (gemm_conv.hip): dispatch thresholds and kernel families */                               \
    X(GEMM_BIG_TILE_MIN, "gemm_big_tile_min", "MI355TTS_BIG_TILE_MIN", ENV_INT, 160, STORE, 0, 0)                       \
    X(GEMM_N192_MIN, "gemm_n192_min", nullptr, ENV_INT, 160, STORE, 0, 0)                                               \
    X(GEMM_MID_TILE_MIN, "gemm_mid_tile_min", nullptr, ENV_INT, 160, STORE, 0, 0)                                       \
    X(GEMM_DMA3_K_MIN, "gemm_dma3_k_min", "MI355TTS_DMA3_K_MIN", ENV_INT, 2048, STORE, 0, 0)                            \
    X(GEMM_USE_DMA3, "gemm_use_dma3", "MI355TTS_NO_DMA3_GEMM", ENV_ONE_OFF, 1, BOOL, 0, 1)                              \
    X(GEMM_USE_DMA, "gemm_use_dma", "MI355TTS_NO_DMA_GEMM", ENV_ONE_OFF, 1, BOOL, 0, 1)                                 \
    X(GEMM_BIG_TILES, "gemm_big_tiles", "MI355TTS_NO_BIG_TILES", ENV_ONE_OFF, 1, BOOL, 0, 1)                            \
    X(GEMM_N192, "gemm_n192", "MI355TTS_NO_N192", ENV_ONE_OFF, 1, BOOL, 0, 1)                                           \
    X(GEMM_F32_DMA, "gemm_f32_dma", nullptr, ENV_INT, 1, BOOL, 0, 1)                                                    \
    X(GEMM_RING4, "gemm_ring4", "MI355TTS_NO_RING4", ENV_ONE_OFF, 1, BOOL, 0, 1)                                        \
    X(GEMM_RING4_MAX, "gemm_ring4_max", "MI355TTS_RING4_MAX", ENV_INT, 256, STORE, 0, 0)                                \
    X(GEMM_BUF, "gemm_buf", "MI355TTS_NO_BUF", ENV_ONE_OFF, 1, BOOL, 0, 1)                                              \
    X(GEMM_F32_SMALL, "gemm_f32_small", "MI355TTS_NO_F32_SMALL", ENV_ONE_OFF, 1, BOOL, 0, 1)                            \
    X(GEMM_F32_SMALL_MAX, "gemm_f32_small_max", "MI355TTS_F32_SMALL_MAX", ENV_INT, 1024, STORE, 0, 0)                   \
    X(GEMM_SMALL16_MAX, "gemm_small16_max", "MI355TTS_SMALL16_MAX", ENV_INT, 256, STORE, 0, 0)                          \
    X(GEMM_F32_N64_DMA, nullptr, "MI355TTS_F32_N64_DMA", ENV_INT, 1, STORE, 0, 0)                                       \
    X(GEMM_N64_DMA16, nullptr, "MI355TTS_N64_DMA16", ENV_INT, 0, STORE, 0, 0) /* 16-bit: neutral (455 vs 457 ms at 8 utterances), off */ \
    X(GEMM_XCD_ORDER, nullptr, "MI355TTS_XCD_ORDER", ENV_ONE_ON, 0, BOOL, 0, 1)                                         \
    X(GEMM_LDS_EPI, nullptr, "MI355TTS_NO_LDS_EPI", ENV_ONE_OFF, 1, BOOL, 0, 1)                                         \
    X(GEMM_ROW_SPLIT, "gemm_row_split", nullptr, ENV_INT, 1, STORE, 0, 0) /* rows beyond the last whole round of 256x256 tiles as a second launch */ \
    /* stream-K (gemm_sk.hip): 0 off, 1 fp32 linear layers, 2 also 16-bit; stages: ring depth override (0 = automatic) */ \
    X(GEMM_SK, "gemm_sk", "MI355TTS_SK", ENV_INT, 1, STORE, 0, 0)                                                       \
    X(GEMM_SK_STAGES, "gemm_sk_stages", "MI355TTS_SK_STAGES", ENV_INT, 0, STORE, 0, 0)                                  \
    X(GEMM_SK_ORDER, nullptr, "MI355TTS_SK_ORDER", ENV_INT, -1, STORE, 0, 0)                                            \
    /* fp32 QKV + RoPE on stream-K: its scatter epilogue is slow and in a persistent launch every workgroup runs it at the same */ \
    /* time at the end (in-model 184 us against 138 us for the 64x64 tiles, whose epilogues overlap other main loops): off */ \
    X(GEMM_SK_QKV32, nullptr, "MI355TTS_SK_QKV32", ENV_INT, 0, STORE, 0, 0)                                             \
    /* fp32 products from 16-bit partial products: gemm_x3.hip, the panel-plane form gemm_x3p.hip, the exact-fit form gemm_x3d.hip */ \
    X(GEMM_F32_X3, "gemm_f32_x3", "MI355TTS_F32_X3", ENV_INT, 1, STORE, 0, 0)                                           \
    X(GEMM_F32_X3P, "gemm_f32_x3p", "MI355TTS_F32_X3P", ENV_INT, 1, STORE, 0, 0)                                        \
    X(GEMM_F32_PLANES, "gemm_f32_planes", "MI355TTS_F32_PLANES", ENV_INT, 2, REJECT, 2, 3) /* panel planes built from now on: 3 bf16 planes | 2 fp16 {hi, lo} */ \
    X(GEMM_F32_N64_PAIRS, "gemm_f32_n64_pairs", nullptr, ENV_INT, 1, STORE, 0, 0) /* fp32 N = 64 convolutions with >= 8 taps: fp16 pairs split in registers */ \
    X(GEMM_F32_GCONV, "gemm_f32_gconv", nullptr, ENV_INT, 1, STORE, 0, 0) /* ... each operand split once per workgroup (gconv_pairs.hip) */ \
    X(GEMM_X3P_NOALIGN, "gemm_x3p_noalign", "MI355TTS_X3P_NOALIGN", ENV_INT, 0, STORE, 0, 0) /* A/B: 1 = no cyclic K alignment */ \
    X(GEMM_X3P_GRID, "gemm_x3p_grid", "MI355TTS_X3P_GRID", ENV_INT, 0, STORE, 0, 0) /* A/B: 0 = automatic, else GR (1, 2, 4, 8) */ \
    X(GEMM_X3D, "gemm_x3d", "MI355TTS_X3D", ENV_INT, 1, STORE, 0, 0) /* 0 off, 1 automatic */                           \
    X(GEMM_X3D_MIN_EFF, "gemm_x3d_min_eff", "MI355TTS_X3D_MIN_EFF", ENV_INT, 90, STORE, 0, 0) /* per cent of useful tile area */ \
    /* gemm_x3d.hip epilogues: which roles store write-through (store16, lds_dma.h).  Bit 0 QKV, 1 FF1, 2 O / FF2, 3 rows / planes */ \
    /* out, 4 attention (reserved: its 8-byte stores stay plain), 5 the fp32 rows of O / FF2 as whole lines with plain stores (A/B). */ \
    /* Default 14: the roles whose period fell in every alternation (profiles/r21/INDEX.md); QKV rose by 0.3 - 1.0 us and stays plain */ \
    X(EPI_WT, nullptr, "MI355TTS_EPI_WT", ENV_INT, 14, CLAMP, 0, 63)                                                    \
    /* 256x256 eight-phase kernel (gemm_ph8.hip) for 16-bit linear layers with at least min_tiles tiles of 256x256 */   \
    X(GEMM_PH8, "gemm_ph8", "MI355TTS_PH8", ENV_INT, 1, STORE, 0, 0)                                                    \
    X(GEMM_PH8_MIN_TILES, "gemm_ph8_min_tiles", "MI355TTS_PH8_MIN", ENV_INT, 200, STORE, 0, 0)                          \
    X(GEMM_PH8_ORDER, "gemm_ph8_order", "MI355TTS_PH8_ORDER", ENV_INT, 1, STORE, 0, 0)                                  \
    /* split tail: measured a gain only for the K = 2048 layer (FF2, 32 K tiles), two slices; the fix-up is unrolled for at most 4 */ \
    X(GEMM_PH8_SPLIT_MAX, "gemm_ph8_split_max", "MI355TTS_PH8_SPLIT", ENV_INT, 2, CLAMP, 1, 4)                          \
    X(GEMM_PH8_SPLIT_MIN_NK, "gemm_ph8_split_min_nk", nullptr, ENV_INT, 24, STORE, 0, 0)                                \
    /* the position convolution's own kernels */                                                                        \
    X(GCONV_TWO_TAPS, "gconv_two_taps", "MI355TTS_GCONV2", ENV_ZERO_OFF, 1, BOOL, 0, 1)                                 \
    X(GCONV16, "gconv16", "MI355TTS_GCONV16", ENV_ZERO_OFF, 1, BOOL, 0, 1)                                              \
    /* attention (attention.hip) */                                                                                     \
    X(ATTN_F32_X3, "attn_f32_x3", "MI355TTS_ATTN_X3", ENV_INT, 2, CLAMP, 0, 2)                                          \
    X(ATTN_F32_PLANES, "attn_f32_planes", "MI355TTS_ATTN_PLANES", ENV_INT, 2, REJECT, 2, 3) /* pre-split K / V^T (and Q / P in the kernel): 2 fp16 pairs | 3 bf16 planes */ \
    X(ATTN_SPLIT, "attn_split", "MI355TTS_ATTN_NO_SPLIT", ENV_ONE_OFF, 2, CLAMP, 0, 2) /* small grids: 1 = 64-query workgroups, keys split between wave pairs (+ key slices); 2 = fp32 pairs kernel: 128-query workgroups + key slices */ \
    X(ATTN_XCD_MAP, "attn_xcd_map", nullptr, ENV_INT, 1, BOOL, 0, 1) /* XCD-aware (query tile, head) map of the workgroup ids (-1 % per launch, bit-neutral) */ \
    X(ATTN_KV_PLANES, "attn_kv_planes", "MI355TTS_ATTN_KVP", ENV_INT, 1, BOOL, 0, 1) /* fp32, both products split: K / V^T pre-split by the QKV epilogue */ \
    X(ATTN_V_ROWS, nullptr, "MI355TTS_ATTN_V_ROWS", ENV_ZERO_OFF, 1, BOOL, 0, 1) /* pre-split V leaves the QKV epilogue as rows like K, transposed on the LDS read; '0': V^T planes (the A/B switch) */ \
    X(ATTN_LPT, "attn_lpt", "MI355TTS_ATTN_LPT", ENV_INT, 1, BOOL, 0, 1) /* fp32 128-query kernel: uneven key slices, longest first */ \
    X(ATTN_Z_FORCE, "attn_z_force", nullptr, ENV_INT, 0, CLAMP, 0, 4) /* tests: exactly that many slices, even empty ones */ \
    /* key slices of the SPLIT2 form: at most Z for fp32, Z16 for 16-bit operands (1 = off: no gain measured) */        \
    X(ATTN_Z, nullptr, "MI355TTS_ATTN_Z", ENV_INT, 4, CLAMP, 1, 4)                                                      \
    X(ATTN_Z16, nullptr, "MI355TTS_ATTN_Z16", ENV_INT, 1, CLAMP, 1, 4)                                                  \
    X(ATTN_CUTS, nullptr, "MI355TTS_ATTN_CUTS", ENV_CUTS, 0, STORE, 0, 0) /* experiments: "7,14" = slices of stages [0,7) [7,14) [14,S) */ \
    /* GPT decode (gpt.hip) */                                                                                          \
    X(GPT_MFMA_MIN, "gpt_mfma_min", nullptr, ENV_INT, 9, STORE, 0, 0) /* sentences from which the batched step uses MFMA */ \
    X(GPT_MFMA, nullptr, "MI355TTS_GPT_NO_MFMA", ENV_ONE_OFF, 1, BOOL, 0, 1)                                            \
    /* BigVGAN (bigvgan.hip, aa_act.hip, aa_conv.hip) */                                                                \
    X(BIGVGAN_STREAMS, "bigvgan_streams", nullptr, ENV_INT, 3, CLAMP, 1, 3)                                             \
    X(BV_SYNC, nullptr, "MI355TTS_BV_SYNC", ENV_ONE_ON, 0, BOOL, 0, 1)                                                  \
    X(AA_TILE, "aa_tile", "MI355TTS_AA_TILE", ENV_INT, 8192, STORE, 0, 0) /* tile size in elements (rows x channels) */   \
    X(AA_PIPE, "aa_pipe", "MI355TTS_AA_PIPE", ENV_ZERO_OFF, 1, BOOL, 0, 1) /* 0: one tile per workgroup (aa_act_kernel) */   \
    X(AA_R, "aa_r", "MI355TTS_AA_R", ENV_INT, 16, STORE, 0, 0) /* outputs per work item of the pipelined kernel; 8: the A/B switch */ \
    X(AACONV_LDS_MIN, "aaconv_lds_min", "MI355TTS_AACONV_LDS_MIN", ENV_INT, 0, STORE, 0, 0) /* > 80 KB: one workgroup per CU (a diagnostic) */

#define MI_OPT_ENUM(name, key, env, conv, dflt, policy, lo, hi) OPT_##name,
enum Opt : int { MI_OPTIONS(MI_OPT_ENUM) OPT_COUNT };

extern std::atomic<long> g_opt[OPT_COUNT];
static inline long opt(Opt o) { return g_opt[o].load(std::memory_order_relaxed); }

void options_init();                                  // the one read of the environment (std::call_once)
bool options_set(const char* key, long v);            // false: unknown key; throws mi::Error (naming the key) for a rejected value
bool options_get(const char* key, long* v);           // false: unknown key
struct AttnCuts { int n = 0; int c[3] = {0, 0, 0}; }; // MI355TTS_ATTN_CUTS as parsed at the one read: n = 0 when unset
const AttnCuts& opt_attn_cuts();

// switches that are not read once (see above): the integer as given or `dflt` when unset; set and first character == c
long env_int(const char* name, long dflt);
bool env_first_is(const char* name, char c);

long option_epoch();              // bumped by every mi_set_option: handles drop their captured hipGraphs when it moved (a graph bakes the dispatch in)
void option_epoch_bump();
std::shared_mutex& option_lock(); // shared: every C-ABI call; exclusive: mi_set_option (capi.hip guard)
}  // namespace mi
