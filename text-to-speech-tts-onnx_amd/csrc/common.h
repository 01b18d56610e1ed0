// common.h — shared host/device helpers for libmi355tts (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <stdexcept>
#include <map>
#include <shared_mutex>

#include "../../include/mi355tts.h"
#include "options.h"

namespace mi {

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
void set_last_error(const std::string& m);

#define MI_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            throw mi::Error(MI_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " @" +   \
                                         __FILE__ + ":" + std::to_string(__LINE__));              \
    } while (0)

#define MI_REQUIRE(cond, msg)                                                                     \
    do {                                                                                          \
        if (!(cond)) throw mi::Error(MI_EINVAL, std::string(msg) + " [" #cond "]");               \
    } while (0)

// ---------------------------------------------------------------------------------------------
// element types.  half = _Float16 ; bf16 = __bf16 (storage) ; all math accumulates in fp32
// ---------------------------------------------------------------------------------------------
using f16 = _Float16;
using bf16 = __bf16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));     // 16 bytes: one lane's share of a b128 load / store / LDS-DMA

template <typename T> struct DT;
template <> struct DT<float> { static constexpr int id = MI_F32; };
template <> struct DT<f16>   { static constexpr int id = MI_F16; };
template <> struct DT<bf16>  { static constexpr int id = MI_BF16; };

inline size_t dtype_size(int dt) { return dt == MI_F32 ? 4 : 2; }

template <typename T> __host__ __device__ inline float to_f32(T v) { return (float)v; }
template <typename T> __host__ __device__ inline T from_f32(float v) { return (T)v; }

// ---------------------------------------------------------------------------------------------
// device buffer (owning)
// ---------------------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; } }
    void ensure(size_t n) {           // grow-only
        if (n <= bytes) return;
        release();
        MI_HIP(hipMalloc(&p, n));
        bytes = n;
    }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// a result to the caller's array (host or device by `mem`; a null array is not wanted), in stream order
inline void copy_out(void* dst, const void* src, size_t bytes, int mem, hipStream_t s) {
    if (!dst) return;
    MI_HIP(hipMemcpyAsync(dst, src, bytes, mem == MI_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
}

// host fp32 -> device tensor of dtype dt
void upload_as(DevBuf& dst, const float* src, size_t n, int dt, hipStream_t s);
void upload_f32(DevBuf& dst, const float* src, size_t n, hipStream_t s);
// compute units of the current device (the launchers size their grids and slices by it): asked once per device, thread-safe;
// 256 (an MI355X) should the runtime report none
int device_cus();

// Reader of a packed fp32 weight blob that lives in host OR device memory (the `mem` flag of mi_*_create_mem; a blob that
// arrived over RCCL stays on the device).  put(): blob range -> device tensor of dtype dt (device blobs: a conversion
// kernel, no host staging).  host(): a host-visible copy of a range, for the few tensors whose load-time tables or
// re-layouts are built by host code.
struct BlobReader {
    int mem; hipStream_t s;
    std::vector<std::vector<float>> keep;
    BlobReader(int mem_, hipStream_t s_) : mem(mem_), s(s_) {}
    const float* host(const float* p, size_t n);
    // dst must already hold >= (dst_off + n) elements when dst_off > 0; with dst_off == 0 it is (re)allocated to n
    void put(DevBuf& dst, const float* p, size_t n, int dt, size_t dst_off = 0);
};

// ---------------------------------------------------------------------------------------------
// profiling (bench roofline leg): HIP events around launches of a kernel family
// ---------------------------------------------------------------------------------------------
struct ProfScope {
    int fam; hipStream_t s; hipEvent_t e0 = nullptr, e1 = nullptr; bool on; double bytes_ = 0, flops_ = 0;
    ProfScope(int family, hipStream_t stream, double bytes, double flops);
    ~ProfScope();
};
enum { FAM_CONV_GEMM = 0, FAM_AA = 1, FAM_CONV_POST = 2, FAM_ATTN = 3, FAM_NORM = 4, FAM_OTHER = 5, FAM_COUNT = 6 };
// per-kernel attribution inside a family: the launcher names the template instantiation it is about to launch (the text
// rocprofv3 --kernel-trace shows for it); the enclosing ProfScope files its elapsed time under that name.  No-op unless
// profiling is on.
void prof_set_kernel(const char* expr, const char* t = nullptr, const char* to = nullptr);
void prof_kernel_suffix(const char* sfx);     // appends to the name prof_set_kernel set last (e.g. a variant of the same launch)
template <typename T> inline const char* type_label();
template <> inline const char* type_label<float>() { return "float"; }
template <> inline const char* type_label<f16>() { return "_Float16"; }
template <> inline const char* type_label<bf16>() { return "__bf16"; }
#define MI_LAUNCH(K, T_, TO_, grid, blk, lds, s, ...)                                                  \
    do {                                                                                               \
        mi::prof_set_kernel(#K, mi::type_label<T_>(), mi::type_label<TO_>());                          \
        hipLaunchKernelGGL(K, grid, blk, lds, s, __VA_ARGS__);                                         \
    } while (0)
void prof_collect();   // resolve pending events (synchronises)
unsigned prof_mask();   // current family mask (0 = profiling off)

// ---------------------------------------------------------------------------------------------
// implicit-GEMM convolution / linear launcher (gemm_conv.hip)
//   out[b, m, n] = epi( sum_{tap, ci} x[b, m - pad + tap*dil, ci] * w[n, tap*Cin + ci] )
// activations are channels-last: element (b, t, c) at  b*bstride + t*rstride + c
// ---------------------------------------------------------------------------------------------
enum Act { ACT_NONE = 0, ACT_GELU_TANH = 1, ACT_GELU_ERF = 2, ACT_MISH = 3, ACT_SILU = 4 };
enum EpiMode { EPI_PLAIN = 0, EPI_CONVT = 1, EPI_QKV_ROPE = 2 };

struct ConvGemm {
    int dtype = MI_F32;           // x / w / res element type
    int out_dtype = -1;           // -1: same as dtype ; MI_F32 allowed
    const void* x = nullptr;
    const void* w = nullptr;      // [G][N][K] , K = taps*Cin contiguous
    const float* bias = nullptr;  // [G*N] (EPI_CONVT: [Cout])
    void* out = nullptr;
    const void* res = nullptr;    // same layout/dtype as out
    const float* gate = nullptr;  // optional per-(b, n) multiplier applied before the residual add
    long gate_bstride = 0;
    int B = 1, G = 1;
    int T_in = 0;                 // valid x rows per batch item
    int M = 0, N = 0, Cin = 0, taps = 1, dil = 1, pad = 0;
    long x_bstride = 0, x_rstride = 0;       // elements
    long out_bstride = 0, out_rstride = 0;   // elements
    long x_goff = 0;              // per-group column offset in x (elements) ; out col offset = g*N
    int act = ACT_NONE;
    float alpha = 1.f;            // out = alpha*(act(acc+bias)*gate + res) (+ out_prev if accumulate)
    int accumulate = 0;
    int epi = EPI_PLAIN;
    // EPI_CONVT: N = u*Cout ; output row tau = m*u + n/Cout - padT, col n%Cout, valid 0<=tau<T_out
    int u = 1, Cout = 0, padT = 0, T_out = 0;
    // EPI_QKV_ROPE (f5): see f5.hip
    const float* rope_cos = nullptr; const float* rope_sin = nullptr; int heads = 0, head_dim = 0;
    const void* rope_pack = nullptr;   // optional: (cos, sin) half pairs [token][head_dim / 2] (values must equal the fp32 tables)
    void* out2 = nullptr; void* out3 = nullptr;
    int rows_per_item = 0;        // EPI_QKV_ROPE with the batch flattened into M: tokens per batch item (0: M)
    int m_off = 0;                // ... and the flattened row this launch's row 0 stands for (row split inside launch_conv_gemm)
    long v_ld = 0;                // > 0: V is written transposed, [b*H + h][head_dim][v_ld] (keys contiguous)
    // fp32 + LDS-staged QKV epilogue only: K and V^T leave as the three bf16 planes of x3_split.h (the attention kernel then
    // stages them without splitting): out2 = [b*H + h][3][k_ld][64], out3 = [b*H + h][3][64][v_ld]; q stays fp32
    int kv_planes = 0; long k_ld = 0;
    int v_rows = 0;               // with kv_planes: V leaves as rows like K, out3 = [b*H + h][np][k_ld][64] (the attention kernel's VROWS form)
    // stream-K workspace of the caller (gemm_sk.hip): sk_slots x 64 KB of partial tiles + sk_slots zero-initialised flags;
    // null: plain linear layers run one tile per workgroup
    float* sk_ws = nullptr; int* sk_flags = nullptr; int sk_slots = 0;
    // fp32 linear layers through the bf16 pipes (gemm_x3.hip): the weights split into three bf16 planes [3][N][K] (split3_planes)
    const void* w3 = nullptr;
    // gemm_x3p.hip (round 3): both operands as pre-split, pre-tiled "panel planes" (x3p_split_rows): xp replaces x, w3p replaces w3
    const void* xp = nullptr; const void* w3p = nullptr; int np = 3;        // np: planes per operand (3 bf16 | 2 fp16), both operands alike
    const void* gcp_w = nullptr;    // gconv_pairs.hip / gconv16.hip: the grouped position convolution's weights as LDS images built at load (fp32: fp16 pairs, gconv_pairs_split_weights; 16-bit: gconv16_build_weights); null: the per-launch kernels
    // ... and its output as panel planes too (the A operand of the NEXT linear layer: FF1 -> FF2), instead of rows in `out`;
    // plain epilogue only: bias + activation, no residual / gate / accumulate
    void* out_planes = nullptr;
    // ---- AdaLN fold (round 4; f5.hip dit_eval; modules.py:301-305,599-613) -------------------------------------------------
    // u = LN(x) * (1 + sc) + sh through W is  rstd * W(x o (1 + sc)) - rstd * mean * (W (1 + sc)) + (W sh + b): the LayerNorm
    // never needs a pass of its own.  PRODUCER (the O / FF2 projections: res + gate epilogue, fp32 rows out): after
    // x_new = res + gate * (acc + bias) it also writes  ln_out = x_new o (1 + ln_scale)  — panel planes of ln_out_np planes
    // (fp32 engines) or rows [M][N] of the engine dtype — and  ln_stats_out[row][N / 32][2] = (sum, M2 about the block mean: wave_reduce.h) of x_new
    // over each 32-column block (plain stores, fixed order: bit-reproducible).  CONSUMER (QKV / FF1): with ln_stats_in set,
    // v = rstd * acc - (mean * rstd) * ln_p[col] + ln_c[col] replaces acc + bias (ln_p = W (1 + sc), ln_c = W sh + b per
    // (step, block), built at load time); mean / rstd over ln_dim columns with ln_eps, biased variance.
    const float* ln_scale = nullptr; void* ln_out = nullptr; float* ln_stats_out = nullptr; int ln_out_np = 0;
    const float* ln_stats_in = nullptr; const float* ln_p = nullptr; const float* ln_c = nullptr; int ln_dim = 0; float ln_eps = 0.f;
    int ln_final = 0;             // consumer: ln_stats_in holds FINISHED (rstd, mean * rstd) per row, [row][2] (launch_ln_finalize), not partials
    // fp16-pair producers: *sat |= 1 when an operand met the fp16 range limit (|a| >= 65504, inf, nan) while being split
    int* sat = nullptr;
    // ragged batches (padded slabs, BigVGAN::run_ragged): output rows >= lens[b] * len_mul + len_add of item b are stored as
    // zeros and tiles wholly past them skip their main loop; lens is a device table of B ints (null: every row is live)
    const int* lens = nullptr; int len_mul = 1, len_add = 0;
    // ... with a bias row per item: item b reads bias[b * bias_bstride + col] (floats; 0: one row for all items).  Launches with
    // lengths only — their direct epilogue is the one that indexes the bias by item; anything else refuses a non-zero stride
    long bias_bstride = 0;
};
constexpr int LN_BLK = 32;        // columns per partial-statistics block of the AdaLN fold
void launch_conv_gemm(const ConvGemm& p, hipStream_t s);
// The launch plan of launch_conv_gemm(p) on a device of `cus` compute units (gemm_conv.hip): the one decision that the dispatch
// switches on and the queries below read.  One kind per family of launch statements.
enum GemmKind { GEMM_NONE = 0, GEMM_DIRECT_256x32, GEMM_DIRECT_128x64, GEMM_DIRECT_128x128, GEMM_DMA64, GEMM_DMA64_PAIRS, GEMM_DMA128,
                GEMM_DMA128_RING4, GEMM_PH8, GEMM_X3P, GEMM_X3, GEMM_SK, GEMM_DMA3_192, GEMM_DMA3_256, GEMM_DMA3_128 };
struct GemmPlan {
    int kind;                                  // GemmKind
    int Tm, Tn, RT, RC, use_buf, lds_epi;      // what ConvGemmDev carries to the kernel under these names (x3p: its launcher tiles it)
    int sk_stages;                             // GEMM_SK: option gemm_sk_stages
    unsigned grid[3];                          // ph8 / x3p / x3 / stream-K size theirs in their own launchers from the CU count: for those kinds a
                                               // mirror that no launch reads (mi_conv_gemm_plan reports it), held by the census fixture only (no ph8 split tail there)
    bool fold_epi;                             // the kind's epilogue carries the AdaLN fold (ln_* fields)
    bool planes_out;                           // ... and may be given out_planes
    int split_rows;                            // > 0: the plan covers the first split_rows rows; the rest is a problem planned by itself
};
void gemm_one_m_axis(ConvGemm& p);              // a one-tap batch over contiguous items becomes one M axis (B = 1): launch_conv_gemm's first step
GemmPlan gemm_plan(const ConvGemm& p, int cus);    // p as given: flatten a batch with gemm_one_m_axis first, as the launch does
bool gemm_ln_fold_ok(const ConvGemm& p, int cus);  // will launch_conv_gemm(p), given the fold's operands, run on kernels whose epilogue has the fold?
// gemm_x3p.hip panel planes: [panel = row / 128][chunk = k / 32][plane 0..2][row % 128][32 bf16], the four 16-byte k-slots of a
// 64-byte row XOR-swizzled by (row >> 2) & 3
constexpr int X3P_PLANE = 128 * 32 * 2;          // one plane of one (panel, chunk): 128 rows x 64 bytes
constexpr int X3P_CHUNK = 3 * X3P_PLANE;         // 24 KB (three bf16 planes)
// Two number formats share the layout (np = planes per operand):
//   np = 3: a = a1 + a2 + a3 in bf16 (x3_split_pair), six partial products per block            -> 2500 / 6 TFLOP/s ceiling
//   np = 2: a = hi + lo * 2^-11 in fp16 (x2_split_pair: 22-bit operands, |a| <= 65504), three partial products per block
//           on two accumulators (hi*hi ; hi*lo + lo*hi)                                          -> 2500 / 3 TFLOP/s ceiling
__host__ __device__ inline int x3p_chunk_bytes(int np) { return np * X3P_PLANE; }
// byte offset of the 16-byte slot holding k = 8 * s8 .. 8 * s8 + 7 of `row` in plane 0 (the other planes: + X3P_PLANE each)
__host__ __device__ inline long x3p_slot_offset(long row, int s8, int nch, int np = 3) {
    const int r = (int)(row & 127);
    return ((row >> 7) * nch + (s8 >> 2)) * (long)(np * X3P_PLANE) + r * 64 + (((s8 & 3) ^ ((r >> 2) & 3)) << 4);
}
long x3p_bytes(long rows, long K, int np = 3);                                        // bytes of the panel planes of a [rows][K] matrix
void x3p_split_rows(const float* x, long ld, void* planes, int rows, int K, hipStream_t s, int np = 3, int* sat = nullptr);   // sat: range watch (x3_split.h)
// gconv_pairs.hip: fp16 {hi, lo} images of a grouped convolution's fp32 weights [G][64][taps][64], one per (group, tap), built once at load
size_t gconv_pairs_planes_bytes(int G, int taps);
void gconv_pairs_split_weights(const float* w, void* wp, int G, int taps, hipStream_t s);
// gconv16.hip: the same convolution on 16-bit engines: weight images [G][taps][64][72] of the engine's type, built once at load
size_t gconv16_image_bytes(int G, int taps);
void gconv16_build_weights(const void* w, int dtype, void* img, int G, int taps, hipStream_t s);
int x3p_planes();                                  // option "gemm_f32_planes": the format new planes are built in (3 or 2)
bool gemm_x3p_enabled();
bool gemm_x3p_would_run(const ConvGemm& p, int cus);        // p.xp / p.w3p set: will launch_conv_gemm(p) take the panel-plane kernel?
bool gemm_x3p_can_write_planes(const ConvGemm& p, int cus); // ... and may it be given out_planes (needs the LDS-staged epilogue: N >= 1024)?
// owner of a stream-K workspace (one per engine handle / stream)
struct SkWorkspace {
    DevBuf ws, flags; int slots = 0;
    void ensure(int n_slots, hipStream_t s);
    void reset(hipStream_t s);       // flags back to zero (after a failed / aborted launch: see F5::recover)
    bool tripped() const;            // the spin watchdog of a stream-K fix-up gave up (last flag word, gemm_x3p.hip): synchronous 4-byte read
    void attach(ConvGemm& g) const { g.sk_ws = ws.as<float>(); g.sk_flags = flags.as<int>(); g.sk_slots = slots; }
};

// How an fp32 engine forms its fp32 products on the matrix cores — a property of the ENGINE, not of the process (VERDICT r3
// weak #1: an fp16-pair engine and a native-fp32 engine must be able to coexist).  The launchers read the process-wide
// options (mi_set_option: tools, A/B runs) THROUGH this thread-local override; every C-ABI call on an F5 handle runs under
// an ArithScope of that handle's setting, so the dispatch (and the hipGraphs captured from it) follow the engine.
// A field of -1 means "no override: the process-wide option".
struct ArithOverride {
    int gemm_x3 = -1;      // fp32 linear layers through the 16-bit pipes at all (0: native v_mfma_f32_32x32x2_f32)
    int gemm_x3p = -1;     // ... with both operands as panel planes (gemm_x3p.hip)
    int planes = -1;       // panel-plane format: 2 = fp16 {hi, lo} pairs, 3 = three bf16 planes (exact, full fp32 exponent range)
    int n64_pairs = -1;    // grouped position convolution as fp16 pairs (conv_gemm_dma_kernel PAIRS)
    int gconv = -1;        // ... with each operand split once per workgroup (gconv_pairs.hip)
    int attn_x3 = -1;      // fp32 attention: 0 native, 1 q.k split, 2 both products split
    int attn_np = -1;      // ... as 2 fp16 pairs | 3 bf16 planes
};
enum { ARITH_DEFAULT = -1, ARITH_NATIVE = 0, ARITH_PAIRS = 2, ARITH_BF16X3 = 3 };
ArithOverride arith_for(int kind);     // ARITH_* -> the override that selects it everywhere (ARITH_DEFAULT: all fields -1)
ArithOverride& arith_tls();
struct ArithScope {
    ArithOverride saved;
    explicit ArithScope(const ArithOverride& a) : saved(arith_tls()) { arith_tls() = a; }
    ~ArithScope() { arith_tls() = saved; }
    ArithScope(const ArithScope&) = delete;
    ArithScope& operator=(const ArithScope&) = delete;
};

// anti-aliased SnakeBeta (aa_act.hip); channels-last (B,T,C) -> (B,T+2*shift,C)
struct AAAct {
    int dtype = MI_F32;
    const void* x = nullptr; void* y = nullptr;
    const float* alpha = nullptr;      // exp(alpha_log)            [C]
    const float* inv_beta = nullptr;   // 1/(exp(beta_log)+1e-9)    [C]
    int B = 1, T = 0, C = 0;
    int post = 0;                      // 1: pad-15 variant, output rows T+30
    // ragged batches: item b holds lens[b] * len_mul + len_add input rows (zeros after them); its output rows past
    // that count (+ 30 with post) are stored as zeros (null: every row is live)
    const int* lens = nullptr; int len_mul = 1, len_add = 0;
};
void launch_aa_act(const AAAct& p, hipStream_t s);
const float* aa_filter_host();         // the 12 kaiser-sinc taps

// fused AA-activation -> Conv1d for C <= 96 (aa_conv.hip); channels-last (B,T,C) -> (B,T,C)
struct AAConv {
    int dtype = MI_F32;
    const void* x = nullptr; const void* w = nullptr;   // w: [co][tap][ci]
    const float* bias = nullptr;
    const float* snake_alpha = nullptr; const float* snake_inv_beta = nullptr;
    void* out = nullptr; const void* res = nullptr;
    int B = 1, T = 0, C = 0, k = 3, dil = 1;
    float alpha = 1.f; int accumulate = 0;
    const int* lens = nullptr; int len_mul = 1, len_add = 0;   // ragged batches, as AAAct
};
void launch_aa_conv(const AAConv& p, hipStream_t s);
void split3_planes(const float* w, void* planes, long n, hipStream_t s);   // gemm_x3.hip
bool gemm_x3_enabled();

// layout helpers (elementwise.hip)
// (B,C,T) fp32 channels-first -> (B,T,Cpad) dtype channels-last (zero padded channels)
void launch_ncl_to_nlc(const float* x, void* y, int B, int C, int T, int Cpad, int dtype, hipStream_t s);
// ragged batches: item b's (C, lens[b]) channels-first array starts at x + C * offs[b] (host-built device tables); it becomes
// slab b of (B, T, Cpad), rows >= lens[b] zero
void launch_ncl_to_nlc_len(const float* x, void* y, int B, int C, int T, int Cpad, int dtype, const int* lens, const long* offs,
                           hipStream_t s);
// (B,T,C) dtype channels-last -> (B,C,T) fp32 channels-first
void launch_nlc_to_ncl(const void* x, float* y, int B, int C, int T, int dtype, hipStream_t s);
// conv_post: (B,T,C) -> tanh/clamp -> float (B,T) and/or int16 (B,T)
void launch_conv_post(const void* x, const float* w /*[7][C]*/, float bias, int B, int T, int C, int dtype,
                      int use_tanh, float* out_f32, int16_t* out_i16, hipStream_t s);
// ragged batches: item b has lens[b] * len_mul + len_add output samples, written from out + offs[b] (the items concatenated)
void launch_conv_post_len(const void* x, const float* w, float bias, int B, int T, int C, int dtype, int use_tanh, float* out_f32,
                          int16_t* out_i16, const int* lens, int len_mul, int len_add, const long* offs, hipStream_t s);
// windows: win[3b ..] = (first kept sample, kept count, output offset) of item b; samples outside the kept range are not written
void launch_conv_post_win(const void* x, const float* w, float bias, int B, int T, int C, int dtype, int use_tanh, float* out_f32,
                          int16_t* out_i16, const int* lens, int len_mul, int len_add, const long* win, hipStream_t s);

}  // namespace mi
