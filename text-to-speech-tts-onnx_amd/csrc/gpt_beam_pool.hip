// gpt_beam_pool.hip — beam search with a pool of finished hypotheses, and beam sampling on top of it: the definition is in
// include/mi355tts.h ("beam search with a finished pool"), this is its device form.  The decode step is gpt_beam.hip's (the
// batched step over nb * B rows, gpt_attn1_beam_kernel over the ancestor table); only the last kernel differs:
//
//   gpt_pool_step_kernel    one 1024-thread workgroup per sentence.  Row lse as gpt_beam_step_kernel; in sampling mode the
//                           per-row top-k / top-p thresholds by the sampler's radix descents (gpt_pick.h), all rows of the group
//                           in the same passes; acc or acc + Gumbel noise of every candidate as an order-preserving uint key
//                           into a scratch row; the K best by a radix descent over (key, ~flat index) — K = (n_stop + 1) * B
//                           is up to 64, too many for beam_choose's per-thread lists — sorted by rank counting in one wave;
//                           stop test, next running hypotheses, pool merge, `open`; then the move of the running hypotheses
//                           as in beam_step_body.
//   gpt_pool_gather_kernel  pool entry 0 along its frozen ancestor list.
// and for pool groups in the sentence queue (gpt_queue.hip): gpt_pool_first_segs_kernel (selection 0 of every group a packed pass
// admitted), gpt_pool_reset_kernel (one group's pool made empty at admission), gpt_pool_out_kernel (retirement by table).
//
// The pool lives in device memory per group (GptPoolDev): an entry is a score, a flag, a length and a physical row that holds
// its frozen ancestor list, its last token and its last last_hidden_state row; the merge permutes the small words and never
// moves a row.  The done flag is GS_DONE of the group's slots, so a captured run of steps replays unchanged.
#include "gpt.h"
#include "gpt_pick.h"
#include "gpt_pool.h"
#include "wave_reduce.h"

namespace mi {

constexpr int POOL_KMAX = GPT_POOL_MAX_CAND;

struct PoolShared {
    float red[16][GPT_BEAM_MAX];
    float lse[GPT_BEAM_MAX], prev[GPT_BEAM_MAX];
    unsigned hist[GPT_BEAM_MAX][256];
    unsigned long long mass[GPT_BEAM_MAX][256];
    unsigned long long wq[16][GPT_BEAM_MAX];
    unsigned sel_bin[GPT_BEAM_MAX], sel_need[GPT_BEAM_MAX], sel_cnt[GPT_BEAM_MAX];
    unsigned long long sel_mass[GPT_BEAM_MAX];
    unsigned cnt[3][GPT_BEAM_MAX];
    unsigned thr_key[GPT_BEAM_MAX];            // sampling mode: code c of row b is kept when key > thr_key[b], or
    int thr_cut[GPT_BEAM_MAX];                 //   key == thr_key[b] and c <= thr_cut[b]
    int wmin[16];
    unsigned long long ck[POOL_KMAX], cs[POOL_KMAX];
    unsigned n_ck;
    // the selection's results
    int cflat[POOL_KMAX], cstop[POOL_KMAX];
    float cacc[POOL_KMAX];
    int run[GPT_BEAM_MAX], parent[GPT_BEAM_MAX], code[GPT_BEAM_MAX];
    float score[GPT_BEAM_MAX];
    float pscore[GPT_BEAM_MAX];
    int pfin[GPT_BEAM_MAX], psrc[GPT_BEAM_MAX];   // psrc: -1 - j = old entry j, q >= 0 = candidate q
    int open, done;
};

struct PoolArgs {
    int B, codes, n, max_new, n_stop;
    int stops[GS_WORDS - GS_STOP0];
    float length_penalty;
    int early_stopping, sampling;
    GptSampleRec rec;
};

__device__ __forceinline__ unsigned long long pool_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// -log(-log u), u = (k24 + 0.5) * 2^-24: both logarithms see an exactly representable argument
__device__ __forceinline__ float pool_gumbel(unsigned k24) {
    const unsigned odd = 2u * k24 + 1u;                                  // u = odd * 2^-25
    const float t = k24 < (1u << 23) ? -logf((float)odd * 0x1p-25f) : -log1pf(-((float)((1u << 25) - odd) * 0x1p-25f));
    return -logf(t);
}

// One selection of a group by the whole workgroup (steps 1-8 of the definition).  lg / pen: the group's first row of logits /
// penalties (pen may be null), rows `codes` apart; keys: B * codes words of scratch; sh.prev, sh.pscore, sh.pfin, sh.open hold the
// state before the selection.  On return the candidates, the running hypotheses, the pool and `open` / `done` are in sh.
__device__ void pool_choose(const float* __restrict__ lg, const float* __restrict__ pen, unsigned* __restrict__ keys,
                            const PoolArgs& a, PoolShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = a.B, codes = a.codes, first = a.n == 0;
    const int R = first ? 1 : B;
    const int K = min((a.n_stop + 1) * B, POOL_KMAX);
    auto zval = [&](int b, int c) {
        const size_t i = (size_t)b * codes + c;
        return __fmul_rn(lg[i], pen ? pen[i] : 1.f);
    };
    // ---- row max and lse: beam_choose's (gpt_beam.hip) ---------------------------------------------------------------------------
    float m[GPT_BEAM_MAX], lse[GPT_BEAM_MAX];
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) m[b] = -INFINITY;
    for (int c = tid; c < codes; c += 1024) {
#pragma unroll
        for (int b = 0; b < GPT_BEAM_MAX; ++b)
            if (b < R) m[b] = fmaxf(m[b], zval(b, c));
    }
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) {
        if (b < R) {
            const float w = wave_max(m[b]);
            if (lane == 0) sh.red[wave][b] = w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) {
        if (b < R) {
            float t = sh.red[0][b];
#pragma unroll
            for (int q = 1; q < 16; ++q) t = fmaxf(t, sh.red[q][b]);
            m[b] = t;
        }
    }
    __syncthreads();
    float s[GPT_BEAM_MAX];
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) s[b] = 0.f;
    for (int c = tid; c < codes; c += 1024) {
#pragma unroll
        for (int b = 0; b < GPT_BEAM_MAX; ++b)
            if (b < R) s[b] += expf(zval(b, c) - m[b]);
    }
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) {
        if (b < R) {
            const float w = wave_sum(s[b]);
            if (lane == 0) sh.red[wave][b] = w;
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < GPT_BEAM_MAX; ++b) {
        lse[b] = 0.f;
        if (b < R) {
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) t += sh.red[q][b];
            lse[b] = m[b] + logf(t);
        }
    }
    if (tid < GPT_BEAM_MAX) {
        float v = 0.f;
#pragma unroll
        for (int b = 0; b < GPT_BEAM_MAX; ++b) v = b == tid ? lse[b] : v;
        sh.lse[tid] = v;
        sh.thr_key[tid] = 0u; sh.thr_cut[tid] = 0x7fffffff;
    }
    if (tid == 0) sh.n_ck = 0;
    __syncthreads();
    const float inv_T = a.rec.inv_T;
    // w of the definition's step 2 (sampling mode: one rounded multiply by inv_T) and acc of step 3, wherever they are formed
    auto wval = [&](int b, int c) {
        const float lp = zval(b, c) - sh.lse[b];
        return a.sampling ? __fmul_rn(lp, inv_T) : lp;
    };
    auto accval = [&](int b, int c) { return first ? wval(b, c) : __fadd_rn(sh.prev[b], wval(b, c)); };

    // ---- sampling mode: the per-row thresholds, the R rows in the same passes -----------------------------------------------------
    if (a.sampling) {
        // count_descent: 4 passes of an 8-bit descent per row, the need0-th largest key of each row counted with multiplicity
        const int top_k = a.rec.top_k;
        const bool use_k = top_k > 0 && top_k < codes, use_p = a.rec.top_p < 1.f;
        unsigned tk[GPT_BEAM_MAX], tp[GPT_BEAM_MAX];
#pragma unroll
        for (int b = 0; b < GPT_BEAM_MAX; ++b) { tk[b] = 0u; tp[b] = 0u; }
        auto count_descent = [&](unsigned need0, unsigned (&out)[GPT_BEAM_MAX]) {
            unsigned prefix[GPT_BEAM_MAX], need[GPT_BEAM_MAX], mask = 0;
#pragma unroll
            for (int b = 0; b < GPT_BEAM_MAX; ++b) { prefix[b] = 0; need[b] = need0; }
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                for (int q = tid; q < R * 256; q += 1024) (&sh.hist[0][0])[q] = 0;
                if (tid < GPT_BEAM_MAX) { sh.sel_bin[tid] = 0; sh.sel_need[tid] = 1; sh.sel_cnt[tid] = 1; }
                __syncthreads();
#pragma unroll
                for (int b = 0; b < GPT_BEAM_MAX; ++b) {
                    if (b < R) {
                        for (int c = tid; c < codes; c += 1024) {
                            const unsigned key = order_key(wval(b, c));
                            if ((key & mask) == prefix[b]) atomicAdd(&sh.hist[b][(key >> shift) & 255u], 1u);
                        }
                    }
                }
                __syncthreads();
                if (wave < R) {
                    unsigned nd = 0;
#pragma unroll
                    for (int b = 0; b < GPT_BEAM_MAX; ++b) nd = b == wave ? need[b] : nd;
                    select_from_top<unsigned>(sh.hist[wave], nd, lane, &sh.sel_bin[wave], &sh.sel_need[wave], &sh.sel_cnt[wave]);
                }
                __syncthreads();
#pragma unroll
                for (int b = 0; b < GPT_BEAM_MAX; ++b) {
                    if (b < R) { prefix[b] |= sh.sel_bin[b] << shift; need[b] = sh.sel_need[b]; }
                }
                mask |= 255u << shift;
                __syncthreads();
            }
#pragma unroll
            for (int b = 0; b < GPT_BEAM_MAX; ++b) out[b] = prefix[b];
        };
        if (use_k) count_descent((unsigned)top_k, tk);
#pragma unroll
        for (int b = 0; b < GPT_BEAM_MAX; ++b) tp[b] = tk[b];
        if (use_p) {
            // e = exp(w - max w) on K in 2^-40 fixed point (the sampler's), S per row
            float wmax[GPT_BEAM_MAX];
            unsigned long long S[GPT_BEAM_MAX];
#pragma unroll
            for (int b = 0; b < GPT_BEAM_MAX; ++b) { wmax[b] = b < R ? __fmul_rn(m[b] - lse[b], inv_T) : 0.f; S[b] = 0ull; }
            auto massval = [&](int b, int c, unsigned& key, float wm, unsigned floor_key) {
                const float w = wval(b, c);
                key = order_key(w);
                return key >= floor_key ? __float2ull_rn(expf(w - wm) * 0x1p40f) : 0ull;
            };
#pragma unroll
            for (int b = 0; b < GPT_BEAM_MAX; ++b) {
                if (b < R) {
                    unsigned long long t = 0;
                    for (int c = tid; c < codes; c += 1024) { unsigned key; t += massval(b, c, key, wmax[b], tk[b]); }
                    t = pool_wave_sum(t);
                    if (lane == 0) sh.wq[wave][b] = t;
                }
            }
            __syncthreads();
            unsigned long long need[GPT_BEAM_MAX];
            int ex;
            const unsigned long long m24 = (unsigned long long)ldexpf(frexpf(a.rec.top_p, &ex), 24);
            const int rs = 24 - ex;
#pragma unroll
            for (int b = 0; b < GPT_BEAM_MAX; ++b) {
                need[b] = 1ull;
                if (b < R) {
                    for (int q = 0; q < 16; ++q) S[b] += sh.wq[q][b];
                    // ceil(top_p * S) in integers, as the sampler forms it
                    const unsigned long long lo = S[b] * m24, hi = __umul64hi(S[b], m24);
                    unsigned long long nd;
                    if (rs < 64) nd = ((hi << (64 - rs)) | (lo >> rs)) + ((lo & ((1ull << rs) - 1ull)) != 0ull);
                    else if (rs < 128) nd = (hi >> (rs - 64)) + (lo != 0ull || (hi & ((1ull << (rs - 64)) - 1ull)) != 0ull);
                    else nd = 1ull;
                    need[b] = nd < 1ull ? 1ull : (nd > S[b] ? S[b] : nd);
                }
            }
            unsigned prefix[GPT_BEAM_MAX], mask = 0;
#pragma unroll
            for (int b = 0; b < GPT_BEAM_MAX; ++b) prefix[b] = 0;
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                for (int q = tid; q < R * 256; q += 1024) (&sh.mass[0][0])[q] = 0ull;
                if (tid < GPT_BEAM_MAX) { sh.sel_bin[tid] = 0; sh.sel_mass[tid] = 1ull; }
                __syncthreads();
#pragma unroll
                for (int b = 0; b < GPT_BEAM_MAX; ++b) {
                    if (b < R) {
                        for (int c = tid; c < codes; c += 1024) {
                            unsigned key;
                            const unsigned long long q = massval(b, c, key, wmax[b], tk[b]);
                            if (q != 0ull && (key & mask) == prefix[b]) atomicAdd(&sh.mass[b][(key >> shift) & 255u], q);
                        }
                    }
                }
                __syncthreads();
                if (wave < R) {
                    unsigned long long nd = 0;
#pragma unroll
                    for (int b = 0; b < GPT_BEAM_MAX; ++b) nd = b == wave ? need[b] : nd;
                    select_from_top<unsigned long long>(sh.mass[wave], nd, lane, &sh.sel_bin[wave], &sh.sel_mass[wave]);
                }
                __syncthreads();
#pragma unroll
                for (int b = 0; b < GPT_BEAM_MAX; ++b) {
                    if (b < R) { prefix[b] |= sh.sel_bin[b] << shift; need[b] = sh.sel_mass[b]; }
                }
                mask |= 255u << shift;
                __syncthreads();
            }
#pragma unroll
            for (int b = 0; b < GPT_BEAM_MAX; ++b) tp[b] = prefix[b] > tk[b] ? prefix[b] : tk[b];
        }
        // a row whose P holds fewer than K codes keeps exactly its K best, ties to the lower code (min_tokens_to_keep = K)
        if (use_p) {
            unsigned kk[GPT_BEAM_MAX];
            count_descent((unsigned)K, kk);
            if (tid < 3 * GPT_BEAM_MAX) (&sh.cnt[0][0])[tid] = 0;
            __syncthreads();
#pragma unroll
            for (int b = 0; b < GPT_BEAM_MAX; ++b) {
                if (b < R) {
                    unsigned np = 0, ng = 0, ne = 0;
                    for (int c = tid; c < codes; c += 1024) {
                        const unsigned key = order_key(wval(b, c));
                        np += key >= tp[b]; ng += key > kk[b]; ne += key == kk[b];
                    }
                    if (np) atomicAdd(&sh.cnt[0][b], np);
                    if (ng) atomicAdd(&sh.cnt[1][b], ng);
                    if (ne) atomicAdd(&sh.cnt[2][b], ne);
                }
            }
            __syncthreads();
            for (int b = 0; b < R; ++b) {                              // uniform: every thread reads the same counts
                const unsigned np = sh.cnt[0][b], ng = sh.cnt[1][b], ne = sh.cnt[2][b];
                unsigned key_b = 0, kk_b = 0;
#pragma unroll
                for (int q = 0; q < GPT_BEAM_MAX; ++q) { key_b = q == b ? tp[q] : key_b; kk_b = q == b ? kk[q] : kk_b; }
                if (np >= (unsigned)K) {                                // P is closed under ties and holds the K best
                    if (tid == 0) { sh.thr_key[b] = key_b; sh.thr_cut[b] = 0x7fffffff; }
                    continue;
                }
                int cut = 0x7fffffff;
                const int need_eq = K - (int)ng;
                if ((int)ne > need_eq) {                                // ties across the K-th place: the need_eq lowest codes
                    int lastc = -1;
                    for (int r = 0; r < need_eq; ++r) {
                        int mine = 0x7fffffff;
                        for (int c = tid; c < codes; c += 1024)
                            if (c > lastc && c < mine && order_key(wval(b, c)) == kk_b) mine = c;
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) mine = min(mine, __shfl_xor(mine, o, 64));
                        if (lane == 0) sh.wmin[wave] = mine;
                        __syncthreads();
                        mine = sh.wmin[0];
#pragma unroll
                        for (int q = 1; q < 16; ++q) mine = min(mine, sh.wmin[q]);
                        lastc = mine;
                        __syncthreads();
                    }
                    cut = lastc;
                }
                if (tid == 0) { sh.thr_key[b] = kk_b; sh.thr_cut[b] = cut; }
            }
        } else if (tid < R) {
            // no top-p: K = {key >= tk} holds top_k >= K codes (or every code)
            unsigned t = 0;
#pragma unroll
            for (int b = 0; b < GPT_BEAM_MAX; ++b) t = b == tid ? tk[b] : t;
            sh.thr_key[tid] = t; sh.thr_cut[tid] = 0x7fffffff;
        }
        __syncthreads();
    }

    // ---- every candidate's key into the scratch row: acc, or acc + Gumbel noise; 0 = not a candidate ----------------------------------
    const int N = R * codes;
#pragma unroll 1
    for (int b = 0; b < R; ++b) {
        const unsigned tkey = sh.thr_key[b];
        const int tcut = sh.thr_cut[b];
        for (int c = tid; c < codes; c += 1024) {
            const int i = b * codes + c;
            float kv = accval(b, c);
            bool in = true;
            if (a.sampling) {
                const unsigned wk = order_key(wval(b, c));
                in = wk > tkey || (wk == tkey && c <= tcut);
                if (in) {                                           // a code the warp left out draws nothing
                    const uint4 r = philox4x32_10((unsigned)a.n, (unsigned)i >> 2, 1u, 0u, a.rec.seed_lo, a.rec.seed_hi);
                    const unsigned word = (i & 3) == 0 ? r.x : (i & 3) == 1 ? r.y : (i & 3) == 2 ? r.z : r.w;
                    kv = __fadd_rn(kv, pool_gumbel(word >> 8));
                }
            }
            unsigned ok = order_key(kv);
            if (!in || !(kv == kv) || ok == 0u) ok = in && kv == kv ? 1u : 0u;
            keys[i] = ok;
        }
    }
    __syncthreads();

    // ---- the K largest of (key, ~i): an 8-bit descent over the key, and over the index only when equal keys lie across the K-th place
    unsigned long long thr = 0;
    {
        unsigned long long prefix = 0, mask = 0;
        unsigned need = (unsigned)K;
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            if (tid < 256) sh.hist[0][tid] = 0;
            if (tid == 0) { sh.sel_bin[0] = 0; sh.sel_need[0] = 1; sh.sel_cnt[0] = 1; }
            __syncthreads();
            for (int i = tid; i < N; i += 1024) {
                const unsigned k = keys[i];
                const unsigned long long comp = ((unsigned long long)k << 32) | (unsigned)~(unsigned)i;
                if (k != 0u && (comp & mask) == prefix) atomicAdd(&sh.hist[0][(unsigned)(comp >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (wave == 0) select_from_top<unsigned>(sh.hist[0], need, lane, &sh.sel_bin[0], &sh.sel_need[0], &sh.sel_cnt[0]);
            __syncthreads();
            prefix |= (unsigned long long)sh.sel_bin[0] << shift;
            mask |= 255ull << shift;
            need = sh.sel_need[0];
            const bool whole = sh.sel_cnt[0] == need;                   // the bin goes in as a whole: nothing below decides
            __syncthreads();
            if (whole) break;
        }
        thr = prefix;
    }
    for (int i = tid; i < N; i += 1024) {
        const unsigned k = keys[i];
        const unsigned long long comp = ((unsigned long long)k << 32) | (unsigned)~(unsigned)i;
        if (k != 0u && comp >= thr) {
            const unsigned at = atomicAdd(&sh.n_ck, 1u);
            if (at < (unsigned)POOL_KMAX) sh.ck[at] = comp;
        }
    }
    __syncthreads();
    const int nk = min((int)sh.n_ck, K);
    // candidate order by rank counting (the composites are distinct), then acc and the stop test of each
    if (wave == 0) {
        if (lane < nk) {
            const unsigned long long mine = sh.ck[lane];
            int rank = 0;
            for (int r = 0; r < nk; ++r) rank += sh.ck[r] > mine;
            sh.cs[rank] = mine;
        }
    }
    __syncthreads();
    if (wave == 0) {
        float acc = -INFINITY;
        int stop = 1;
        if (lane < K) {
            // fewer than K candidates compare (NaN logits): the rest repeat code 0 of row 0 and count as stopped
            const int i = lane < nk ? (int)~(unsigned)(sh.cs[lane] & 0xffffffffull) : 0;
            const int fi = min(max(i, 0), N - 1), b = fi / codes, c = fi % codes;
            acc = accval(b, c);
            stop = lane >= nk || a.n + 1 >= a.max_new;
#pragma unroll
            for (int q = 0; q < GS_WORDS - GS_STOP0; ++q) stop |= (q < a.n_stop && a.stops[q] == c);
            sh.cflat[lane] = fi; sh.cacc[lane] = acc; sh.cstop[lane] = stop;
        }
        if (lane < GPT_BEAM_MAX) sh.run[lane] = -1;
    }
    __syncthreads();
    if (wave == 0) {
        // step 6: the B live candidates of largest acc, ties to the earlier one
        const float acc = lane < K ? sh.cacc[lane] : -INFINITY;
        if (lane < K && !sh.cstop[lane]) {
            int rank = 0;
            for (int r = 0; r < K; ++r) {
                const float ov = sh.cacc[r];
                rank += !sh.cstop[r] && (ov > acc || (ov == acc && r < lane));
            }
            if (rank < B) sh.run[rank] = lane;
        }
        // steps 7 and 8 on items 0 .. B-1 = the pool, B .. 2B-1 = the first B candidates
        const float scale = powf((float)(a.n + 1), a.length_penalty);
        bool full = true;
        for (int j = 0; j < B; ++j) full &= sh.pfin[j] != 0;
        const bool admit = sh.open && !(a.early_stopping && full);
        float v = 0.f;
        bool valid = false;
        if (lane < B) { v = sh.pscore[lane]; valid = true; }
        else if (lane < 2 * B && lane - B < K) { v = sh.cacc[lane - B] / scale; valid = admit && sh.cstop[lane - B] && lane - B < nk; }
        int rank = 0;
        for (int r = 0; r < 2 * B; ++r) {
            const float ov = __shfl(v, r, 64);
            const bool ovalid = __shfl((int)valid, r, 64) != 0;
            rank += ovalid && (ov > v || (ov == v && r < lane));
        }
        float nscore[GPT_BEAM_MAX];
        int nfin[GPT_BEAM_MAX], nsrc[GPT_BEAM_MAX];
        const int fin = lane < B ? sh.pfin[lane] : 1;
        const int src = lane < B ? -1 - lane : lane - B;
#pragma unroll
        for (int j = 0; j < GPT_BEAM_MAX; ++j) {
            const unsigned long long hit = __ballot(valid && rank == j);
            const int from = hit ? __ffsll((long long)hit) - 1 : 0;
            nscore[j] = __shfl(v, from, 64); nfin[j] = __shfl(fin, from, 64); nsrc[j] = __shfl(src, from, 64);
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < GPT_BEAM_MAX; ++j)
                if (j < B) { sh.pscore[j] = nscore[j]; sh.pfin[j] = nfin[j]; sh.psrc[j] = nsrc[j]; }
        }
    }
    __syncthreads();
    if (tid == 0) {
        bool nfull = true;
        float lowest = INFINITY;
        for (int j = 0; j < B; ++j) { nfull &= sh.pfin[j] != 0; lowest = fminf(lowest, sh.pscore[j]); }
        int open = sh.open;
        const int r0 = sh.run[0];
        if (nfull && r0 >= 0) open = open && (sh.cacc[r0] / powf((float)(a.n + 1), a.length_penalty) > lowest);
        sh.open = open;
        sh.done = !open || (a.early_stopping && nfull) || a.n + 1 >= a.max_new;
    }
    __syncthreads();
    if (tid < B) {
        const int q = sh.run[tid] >= 0 ? sh.run[tid] : 0;              // no live candidate is left only at the limit
        sh.parent[tid] = sh.cflat[q] / codes;
        sh.code[tid] = sh.cflat[q] % codes;
        sh.score[tid] = sh.cacc[q];
    }
    __syncthreads();
}

// mi_gpt_beam_pool_select: one group, the whole state passed in and out
__global__ __launch_bounds__(1024) void gpt_pool_select_kernel(const float* __restrict__ logits, const float* __restrict__ pen,
                                                               unsigned* __restrict__ keys, PoolArgs a,
                                                               const float* __restrict__ prev, float* pool_score, int32_t* pool_fin,
                                                               int32_t* open_done, int32_t* cand, float* cand_acc,
                                                               int32_t* cand_stop, int32_t* parents, int32_t* tokens, float* scores,
                                                               int32_t* pool_src) {
    __shared__ PoolShared sh;
    const int tid = threadIdx.x;
    if (tid < a.B) { sh.prev[tid] = a.n == 0 ? 0.f : prev[tid]; sh.pscore[tid] = pool_score[tid]; sh.pfin[tid] = pool_fin[tid] != 0; }
    if (tid == 0) sh.open = open_done[0] != 0;
    __syncthreads();
    pool_choose(logits, pen, keys, a, sh);
    const int K = min((a.n_stop + 1) * a.B, POOL_KMAX);
    if (tid < K) { cand[tid] = sh.cflat[tid]; cand_acc[tid] = sh.cacc[tid]; cand_stop[tid] = sh.cstop[tid]; }
    if (tid < a.B) {
        parents[tid] = sh.run[tid] >= 0 ? sh.parent[tid] : -1;
        tokens[tid] = sh.run[tid] >= 0 ? sh.code[tid] : -1;
        scores[tid] = sh.score[tid];
        pool_score[tid] = sh.pscore[tid]; pool_fin[tid] = sh.pfin[tid]; pool_src[tid] = sh.psrc[tid];
    }
    if (tid == 0) { open_done[0] = sh.open; open_done[1] = sh.done; }
}

// One pool-mode selection of the group whose first slot is s0: pool_choose, the new pool entries frozen, then beam_step_body's
// move of the running hypotheses (gpt_beam.hip) — a running hypothesis never holds a stop id, so its token is always penalised.
__device__ __forceinline__ void pool_step_body(const float* __restrict__ logits, float* pen0, float* pen1,
                                               const float* __restrict__ last, int* st, int* toks, float* __restrict__ hid,
                                               int* anc0, int* anc1, float* scores, int codes, int hidden, int rows,
                                               const float* __restrict__ rep_dev, int max_tok, const float* __restrict__ emb,
                                               const float* __restrict__ pos, int max_pos, float* __restrict__ xb, int B,
                                               const GptPoolDev& pd, size_t s0) {
    __shared__ PoolShared sh;
    __shared__ int sw[GPT_BEAM_MAX][GS_WORDS];
    __shared__ int pw_r[GPT_BEAM_MAX], new_reset[GPT_BEAM_MAX];
    __shared__ int plen[GPT_BEAM_MAX], prow[GPT_BEAM_MAX], nlen[GPT_BEAM_MAX], nrow[GPT_BEAM_MAX];
    const int tid = threadIdx.x;
    if (tid < B * GS_WORDS) sw[tid / GS_WORDS][tid % GS_WORDS] = st[s0 * GS_WORDS + tid];
    if (tid < B) {
        sh.prev[tid] = scores[s0 + tid];
        sh.pscore[tid] = pd.score[s0 + tid];
        const int* mw = pd.meta + (s0 + tid) * GPT_POOL_META;
        sh.pfin[tid] = mw[PM_FIN] != 0; plen[tid] = mw[PM_LEN]; prow[tid] = min(max(mw[PM_ROW], 0), B - 1);
    }
    if (tid == 0) sh.open = pd.meta[s0 * GPT_POOL_META + PM_OPEN] != 0;
    const float repv = rep_dev[0];
    const GptPoolCfg cf = pd.cfg[0];
    __syncthreads();
    if (sw[0][GS_DONE]) return;                                    // the sentence is done: the step is a no-op (uniform)
    const int n = sw[0][GS_NDEC];
    PoolArgs a;
    a.B = B; a.codes = codes; a.n = n; a.max_new = sw[0][GS_LIMIT];
    a.n_stop = min(max(sw[0][GS_NSTOP], 0), GS_WORDS - GS_STOP0);
#pragma unroll
    for (int q = 0; q < GS_WORDS - GS_STOP0; ++q) a.stops[q] = sw[0][GS_STOP0 + q];
    a.length_penalty = cf.length_penalty; a.early_stopping = cf.early_stopping; a.sampling = cf.sampling;
    a.rec = pd.recs[s0];
    const float* pen_old = ((n & 1) ? pen1 : pen0) + s0 * codes;
    float* pen_new = ((n & 1) ? pen0 : pen1) + s0 * codes;
    const int* anc_old = ((n & 1) ? anc1 : anc0) + s0 * max_tok;
    int* anc_new = ((n & 1) ? anc0 : anc1) + s0 * max_tok;
    pool_choose(logits + s0 * codes, pen_old, pd.keys + s0 * codes, a, sh);
    // ---- the pool: kept entries keep their physical rows, new ones take the rows of the entries that left ----------------------------
    if (tid == 0) {
        unsigned used = 0;
        for (int j = 0; j < B; ++j)
            if (sh.psrc[j] < 0) used |= 1u << prow[-1 - sh.psrc[j]];
        for (int j = 0; j < B; ++j) {
            if (sh.psrc[j] < 0) { nrow[j] = prow[-1 - sh.psrc[j]]; nlen[j] = plen[-1 - sh.psrc[j]]; }
            else {
                int r = 0;
                while (r < B - 1 && (used >> r & 1u)) ++r;
                used |= 1u << r;
                nrow[j] = r; nlen[j] = n + 1;
            }
        }
    }
    __syncthreads();
    const int nprev = min(max(n, 0), max_tok);
    for (int j = 0; j < B; ++j) {
        const int q = sh.psrc[j];
        if (q < 0) continue;                                        // uniform
        const int fi = sh.cflat[min(q, POOL_KMAX - 1)], p = min(max(fi / codes, 0), B - 1), t = fi % codes;
        const size_t row = s0 + nrow[j];
        for (int k = tid; k < nprev; k += 1024) pd.anc[row * max_tok + k] = anc_old[(size_t)p * max_tok + k];
        for (int c = tid; c < hidden; c += 1024) pd.hid[row * hidden + c] = last[(s0 + p) * hidden + c];
        if (tid == 0) pd.meta[row * GPT_POOL_META + PM_TOK] = t;
    }
    if (tid < B) {
        pd.score[s0 + tid] = sh.pscore[tid];
        int* mw = pd.meta + (s0 + tid) * GPT_POOL_META;
        mw[PM_FIN] = sh.pfin[tid]; mw[PM_LEN] = nlen[tid]; mw[PM_ROW] = nrow[tid];
    }
    if (tid == 0) pd.meta[s0 * GPT_POOL_META + PM_OPEN] = sh.open;
    // ---- the running hypotheses move (beam_step_body) ----------------------------------------------------------------------------------
    if (tid < B) {
        const int i = tid, p = min(max(sh.parent[i], 0), B - 1), t = min(max(sh.code[i], 0), codes - 1);
        const int* w = sw[p];
        if (n >= 0 && n < max_tok) toks[(s0 + i) * max_tok + n] = t;
        int wr = -1, reset = w[GS_RESET];
        if (w[GS_UPDATE_PEN]) {
            const int r = reset;
            int tr = 0;
            if (r == n) tr = t;
            else if (r >= 0 && r < n && r < max_tok) {
                const int an = min(max(anc_old[(size_t)p * max_tok + r], 0), B - 1);
                tr = min(max(toks[(s0 + an) * max_tok + r], 0), codes - 1);
            }
            if (n + 1 > w[GS_RANGE] && r < max_tok && tr != t) { wr = tr; reset = r + 1; }
        }
        pw_r[i] = wr; new_reset[i] = reset;
    }
    __syncthreads();
    const int gen = sw[0][GS_GEN_LEN] + 1;
    if (tid < B) {
        const int i = tid, p = min(max(sh.parent[i], 0), B - 1);
        int w[GS_WORDS];
#pragma unroll
        for (int q = 0; q < GS_WORDS; ++q) w[q] = sw[p][q];
        w[GS_TOKEN] = min(max(sh.code[i], 0), codes - 1);
        w[GS_NDEC] = n + 1;
        w[GS_RESET] = new_reset[i];
        w[GS_HIST] += rows;
        w[GS_GEN_LEN] = gen;
        w[GS_DONE] = sh.done;
        int* so = st + (s0 + i) * GS_WORDS;
#pragma unroll
        for (int q = 0; q < GS_STOP0; q += 4) *reinterpret_cast<int4*>(so + q) = make_int4(w[q], w[q + 1], w[q + 2], w[q + 3]);
        if (GS_STOP0 % 4) { for (int q = GS_STOP0 / 4 * 4; q < GS_STOP0; ++q) so[q] = w[q]; }
        scores[s0 + i] = sh.score[i];
        if (n >= 0 && n < max_tok) anc_new[(size_t)i * max_tok + n] = i;
    }
    const int g = min(max(gen, 0), max_pos - 1);
    for (int i = 0; i < B; ++i) {
        const int p = min(max(sh.parent[i], 0), B - 1), t = min(max(sh.code[i], 0), codes - 1);
        const int wt = sw[p][GS_UPDATE_PEN] ? t : -1, wr = pw_r[i];
        for (int c = tid; c < codes; c += 1024) {
            float v = pen_old[(size_t)p * codes + c];
            v = c == wt ? repv : v;
            v = c == wr ? 1.f : v;
            pen_new[(size_t)i * codes + c] = v;
        }
        for (int q = tid; q < nprev; q += 1024) anc_new[(size_t)i * max_tok + q] = anc_old[(size_t)p * max_tok + q];
        for (int c = tid; c < hidden; c += 1024) {
            if (n >= 0 && n < max_tok) hid[((s0 + i) * max_tok + n) * hidden + c] = last[(s0 + p) * hidden + c];
            xb[(s0 + i) * hidden + c] = emb[(size_t)t * hidden + c] + pos[(size_t)g * hidden + c];
        }
    }
}

__global__ __launch_bounds__(1024) void gpt_pool_step_kernel(const float* __restrict__ logits, float* pen0, float* pen1,
                                                             const float* __restrict__ last, int* st, int* toks,
                                                             float* __restrict__ hid, int* anc0, int* anc1, float* scores,
                                                             int codes, int hidden, int rows, const float* __restrict__ rep_dev,
                                                             int max_tok, const float* __restrict__ emb,
                                                             const float* __restrict__ pos, int max_pos, float* __restrict__ xb,
                                                             int B, GptPoolDev pd, int group0) {
    pool_step_body(logits, pen0, pen1, last, st, toks, hid, anc0, anc1, scores, codes, hidden, rows, rep_dev, max_tok, emb, pos,
                   max_pos, xb, B, pd, (size_t)(group0 + blockIdx.x) * B);
}

// The sentence queue in pool mode: selection 0 of every group a packed prompt pass admitted, in one launch — the form of
// gpt_beam_first_segs_kernel (gpt_beam.hip).  Workgroup q serves segment q of the pass's table (Gpt::Seg as an int4: first packed
// row, rows, slot, pad); the group is slot / B and `rows` is the segment's.  A segment whose slot does not name a whole group
// inside the handle's slots is left alone (block-uniform).
__global__ __launch_bounds__(1024) void gpt_pool_first_segs_kernel(const int4* __restrict__ segs, const float* __restrict__ logits,
                                                                   float* pen0, float* pen1, const float* __restrict__ last,
                                                                   int* st, int* toks, float* __restrict__ hid, int* anc0,
                                                                   int* anc1, float* scores, int codes, int hidden,
                                                                   const float* __restrict__ rep_dev, int max_tok,
                                                                   const float* __restrict__ emb, const float* __restrict__ pos,
                                                                   int max_pos, float* __restrict__ xb, int B, GptPoolDev pd,
                                                                   int max_batch) {
    const int4 g = segs[blockIdx.x];
    const int group = g.z / B;
    if (g.z < 0 || (group + 1) * B > max_batch) return;
    pool_step_body(logits, pen0, pen1, last, st, toks, hid, anc0, anc1, scores, codes, hidden, min(max(g.y, 0), max_tok), rep_dev,
                   max_tok, emb, pos, max_pos, xb, B, pd, (size_t)group * B);
}

// The pool of the group whose first slot is s0 made empty for the sentence the queue admits into it (Gpt::pool_begin's state, for
// one group, in stream order): scores -1e9, no entry finished, entry j in physical row j, `open`, and the sentence's record.
__global__ __launch_bounds__(64) void gpt_pool_reset_kernel(float* __restrict__ score, int* __restrict__ meta,
                                                            GptSampleRec* __restrict__ recs, int s0, int B, GptSampleRec rec) {
    const int j = threadIdx.x;
    if (j >= B) return;
    score[s0 + j] = -1.0e9f;
    int* mw = meta + (size_t)(s0 + j) * GPT_POOL_META;
#pragma unroll
    for (int q = 0; q < GPT_POOL_META; ++q) mw[q] = 0;
    mw[PM_ROW] = j;
    mw[PM_OPEN] = 1;
    recs[s0 + j] = rec;
}

// pool entry 0 of every group along its frozen ancestor list; its last token and row are the entry's own
__global__ __launch_bounds__(256) void gpt_pool_gather_kernel(GptPoolDev pd, const int* __restrict__ toks,
                                                              const float* __restrict__ hid, int32_t* __restrict__ tokens,
                                                              float* __restrict__ hidden_out, int B, int max_tok, int hidden,
                                                              int cap) {
    const size_t s0 = (size_t)blockIdx.y * B;
    const int n = blockIdx.x;
    const int* mw = pd.meta + s0 * GPT_POOL_META;
    const int len = mw[PM_FIN] ? mw[PM_LEN] : 0;
    if (n >= len || n >= cap || n >= max_tok) return;
    const size_t row = s0 + min(max(mw[PM_ROW], 0), B - 1);
    const bool own = n == len - 1;
    const size_t src = own ? row : s0 + min(max(pd.anc[row * max_tok + n], 0), B - 1);
    if (tokens && threadIdx.x == 0)
        tokens[(size_t)blockIdx.y * cap + n] = own ? pd.meta[row * GPT_POOL_META + PM_TOK] : toks[src * max_tok + n];
    if (hidden_out)
        for (int c = threadIdx.x; c < hidden; c += 256)
            hidden_out[((size_t)blockIdx.y * cap + n) * hidden + c] = own ? pd.hid[row * hidden + c] : hid[(src * max_tok + n) * hidden + c];
}

// Retirement of the queue's pool groups by table, in the form of gpt_beam_out_kernel (gpt_beam.hip) with the gather above as
// its source: entry q = (slot = the group's first slot, sentence, count, dst_row).  Pool entry 0 of the group leaves: token n
// and last_hidden_state row n below its last along the frozen list pool_anc of its physical row, the last token and row from
// PM_TOK / pool_hid of that row; they go to row dst_row + n of the destination arrays and its score (0 when the pool holds no
// finished entry) to score_dst[sentence].  One block per (row of the longest entry, entry); indices are clamped as above.
__global__ __launch_bounds__(256) void gpt_pool_out_kernel(Gpt::OutTable tab, GptPoolDev pd, const int* __restrict__ toks,
                                                           const float* __restrict__ hid, int32_t* __restrict__ tokens_dst,
                                                           float* __restrict__ hidden_dst, float* __restrict__ score_dst, int B,
                                                           int max_tok, int hidden, int max_batch) {
    const Gpt::OutSeg g = tab.e[blockIdx.y];
    const int n = blockIdx.x;
    if (g.slot < 0 || g.slot % B != 0 || g.slot + B > max_batch || g.sentence < 0) return;      // block-uniform
    const size_t s0 = (size_t)g.slot;
    const int* mw = pd.meta + s0 * GPT_POOL_META;
    const int fin = mw[PM_FIN];
    if (n == 0 && threadIdx.x == 0 && score_dst) score_dst[g.sentence] = fin ? pd.score[s0] : 0.f;
    const int len = fin ? mw[PM_LEN] : 0;
    if (n >= g.count || n >= len || n >= max_tok) return;
    const size_t row = s0 + min(max(mw[PM_ROW], 0), B - 1);
    const bool own = n == len - 1;
    const size_t src = own ? row : s0 + min(max(pd.anc[row * max_tok + n], 0), B - 1);
    const size_t dst = (size_t)(g.dst_row + n);
    if (tokens_dst && threadIdx.x == 0) tokens_dst[dst] = own ? pd.meta[row * GPT_POOL_META + PM_TOK] : toks[src * max_tok + n];
    if (hidden_dst)
        for (int c = threadIdx.x; c < hidden; c += 256)
            hidden_dst[dst * hidden + c] = own ? pd.hid[row * hidden + c] : hid[(src * max_tok + n) * hidden + c];
}

// ---------------------------------------------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------------------------------------------
void launch_gpt_pool_select(const float* logits, const float* pen, unsigned* keys, const GptPoolSelect& p, const float* prev,
                            float* pool_score, int32_t* pool_fin, int32_t* open_done, int32_t* cand, float* cand_acc,
                            int32_t* cand_stop, int32_t* parents, int32_t* tokens, float* scores, int32_t* pool_src, hipStream_t s) {
    MI_REQUIRE(p.codes >= 1 && p.codes <= GPT_BEAM_MAX_CODES, "gpt beam pool: the unit entry supports 1..16384 codes");
    MI_REQUIRE(p.B >= 1 && p.B <= GPT_BEAM_MAX && p.n_stop >= 0 && p.n_stop <= GS_WORDS - GS_STOP0, "gpt beam pool: beams / stop ids");
    MI_REQUIRE((p.n_stop + 1) * p.B <= GPT_POOL_MAX_CAND && (p.n_stop + 1) * p.B <= p.codes, "gpt beam pool: (n_stop + 1) * num_beams must be <= 64 and <= codes");
    MI_REQUIRE(logits && keys && (p.n == 0 || prev) && pool_score && pool_fin && open_done && cand && cand_acc && cand_stop &&
               parents && tokens && scores && pool_src, "gpt beam pool: selection launch");
    PoolArgs a{};
    a.B = p.B; a.codes = p.codes; a.n = p.n; a.max_new = p.max_new; a.n_stop = p.n_stop;
    for (int q = 0; q < p.n_stop; ++q) a.stops[q] = p.stops[q];
    a.length_penalty = p.length_penalty; a.early_stopping = p.early_stopping; a.sampling = p.sampling;
    a.rec = p.rec;
    hipLaunchKernelGGL(gpt_pool_select_kernel, dim3(1), dim3(1024), 0, s, logits, pen, keys, a, prev, pool_score, pool_fin, open_done,
                       cand, cand_acc, cand_stop, parents, tokens, scores, pool_src);
    MI_HIP(hipGetLastError());
}

void Gpt::pool_ensure() {
    beam_ensure();
    if (pool_score.p) return;
    const size_t P = MBp;
    pool_score.ensure(P * 4);
    pool_meta.ensure(P * GPT_POOL_META * 4);
    pool_anc.ensure(P * cfg.max_seq * 4);
    pool_hid.ensure(P * cfg.hidden * 4);
    pool_keys.ensure(P * cfg.mel_codes * 4);
    pool_cfg.ensure(sizeof(GptPoolCfg));
    pool_rec.ensure(P * sizeof(GptSampleRec));
    for (DevBuf* b : {&pool_score, &pool_meta, &pool_anc, &pool_hid, &pool_keys, &pool_cfg, &pool_rec})
        MI_HIP(hipMemsetAsync(b->p, 0, b->bytes, stream));
}

GptPoolDev Gpt::pool_dev() {
    return {pool_score.as<float>(), pool_meta.as<int>(), pool_anc.as<int>(), pool_hid.as<float>(), pool_keys.as<unsigned>(),
            pool_cfg.as<GptPoolCfg>(), pool_rec.as<GptSampleRec>()};
}

// the state of nb empty pools, the call's parameters and (sampling mode) each sentence's record at its group's first slot
void Gpt::pool_begin(int nb, int B, const GptPoolCfg& cf, const GptSampleRec* recs) {
    MI_REQUIRE(nb >= 1 && B >= 1 && nb * B <= cfg.max_batch && pool_score.p, "gpt beam pool: batch exceeds max_batch");
    const int nr = nb * B;
    std::vector<float> sc((size_t)nr, -1.0e9f);
    std::vector<int32_t> meta((size_t)nr * GPT_POOL_META, 0);
    std::vector<GptSampleRec> rc((size_t)nr);
    for (int r = 0; r < nr; ++r) {
        meta[(size_t)r * GPT_POOL_META + PM_ROW] = r % B;
        meta[(size_t)r * GPT_POOL_META + PM_OPEN] = 1;
        rc[r] = recs ? recs[r / B] : GptSampleRec{1.f, 1.f, 0, 0u, 0u, {0u, 0u, 0u}};
    }
    MI_HIP(hipMemcpyAsync(pool_score.p, sc.data(), sc.size() * 4, hipMemcpyHostToDevice, stream));
    MI_HIP(hipMemcpyAsync(pool_meta.p, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, stream));
    MI_HIP(hipMemcpyAsync(pool_rec.p, rc.data(), rc.size() * sizeof(GptSampleRec), hipMemcpyHostToDevice, stream));
    MI_HIP(hipMemcpyAsync(pool_cfg.p, &cf, sizeof(cf), hipMemcpyHostToDevice, stream));
    MI_HIP(hipStreamSynchronize(stream));
}

static void pool_step_launch(Gpt& e, int groups, int group0, int B, int rows) {
    const GptCfg& c = e.cfg;
    MI_REQUIRE(B >= 1 && B <= GPT_BEAM_MAX && B <= c.mel_codes && group0 >= 0 && groups >= 1 &&
               (group0 + groups) * B <= c.max_batch && e.pen_b.p && e.pool_score.p, "gpt beam pool: selection launch");
    int* anc0 = e.anc.as<int>();
    hipLaunchKernelGGL(gpt_pool_step_kernel, dim3(groups), dim3(1024), 0, e.stream, e.logits.as<float>(), e.pen.as<float>(),
                       e.pen_b.as<float>(), e.last.as<float>(), e.state.as<int>(), e.toks.as<int>(), e.hid.as<float>(), anc0,
                       anc0 + (size_t)e.MBp * c.max_seq, e.score.as<float>(), c.mel_codes, c.hidden, rows,
                       e.rep_dev.as<float>(), c.max_seq, e.mel_emb.as<float>(), e.mel_pos.as<float>(), c.max_mel_pos,
                       e.Xd.as<float>(), B, e.pool_dev(), group0);
    MI_HIP(hipGetLastError());
}

void Gpt::pool_select_first(int group, int B, int rows) { pool_step_launch(*this, 1, group, B, rows); }

void Gpt::decode_pool_eager(int nb, int B) {
    const int nr = nb * B;
    MI_REQUIRE(nb >= 1 && B >= 1 && nr <= cfg.max_batch && pen_b.p && pool_score.p, "gpt beam pool: batch exceeds max_batch");
    const int* anc0 = anc.as<int>();
    const int* anc1 = anc0 + (size_t)MBp * cfg.max_seq;
    decode_rows_eager(nr, [&](char* kcl, char* vcl) {
        launch_gpt_attn1_beam(dtype, qkvd.p, kcl, vcl, attd.p, state.as<int>(), anc0, anc1, cfg.heads, nr, cfg.hidden, cfg.max_seq,
                              slot_cache_elems(), B, stream);
    }, [&] { pool_step_launch(*this, nb, 0, B, 1); });
}

void Gpt::decode_pool_steps(int nb, int B, int n) {
    check_graph_epoch();
    replay(batch_graphs[{nb * B, 1 + GPT_BEAM_MAX + B}], n, [&] { decode_pool_eager(nb, B); });
}

void Gpt::pool_gather(int nb, int B, int32_t* tokens, float* hidden, int cap) {
    MI_REQUIRE(nb >= 1 && B >= 1 && nb * B <= cfg.max_batch && cap >= 1 && pool_score.p, "gpt beam pool: gather");
    const int rows = cap < cfg.max_seq ? cap : cfg.max_seq;
    hipLaunchKernelGGL(gpt_pool_gather_kernel, dim3(rows, nb), dim3(256), 0, stream, pool_dev(), toks.as<int>(), hid.as<float>(),
                       tokens, hidden, B, cfg.max_seq, cfg.hidden, cap);
    MI_HIP(hipGetLastError());
}

// the call's parameters alone (a queue session has one GptPoolCfg; its groups are reset one by one, pool_reset_group)
void Gpt::pool_set_cfg(const GptPoolCfg& cf) {
    MI_REQUIRE(pool_cfg.p, "gpt beam pool: parameters before pool_ensure");
    MI_HIP(hipMemcpyAsync(pool_cfg.p, &cf, sizeof(cf), hipMemcpyHostToDevice, stream));
    MI_HIP(hipStreamSynchronize(stream));
}

void Gpt::pool_reset_group(int group, int B, const GptSampleRec* rec) {
    MI_REQUIRE(B >= 1 && B <= GPT_BEAM_MAX && group >= 0 && (group + 1) * B <= cfg.max_batch && pool_score.p, "gpt beam pool: group reset");
    const GptSampleRec r = rec ? *rec : GptSampleRec{1.f, 1.f, 0, 0u, 0u, {0u, 0u, 0u}};
    hipLaunchKernelGGL(gpt_pool_reset_kernel, dim3(1), dim3(64), 0, stream, pool_score.as<float>(), pool_meta.as<int>(),
                       pool_rec.as<GptSampleRec>(), group * B, B, r);
    MI_HIP(hipGetLastError());
}

// selection 0 of the k pool groups whose segments forward_packed left in segtab, one launch
void Gpt::pool_select_segs(int k, int B) {
    const GptCfg& c = cfg;
    MI_REQUIRE(B >= 1 && B <= GPT_BEAM_MAX && B <= c.mel_codes && k >= 1 && k * B <= c.max_batch && pen_b.p && pool_score.p && segtab.p,
               "gpt beam pool: selection launch over a pass's segments");
    int* anc0 = anc.as<int>();
    hipLaunchKernelGGL(gpt_pool_first_segs_kernel, dim3(k), dim3(1024), 0, stream, segtab.as<int4>(), logits.as<float>(),
                       pen.as<float>(), pen_b.as<float>(), last.as<float>(), state.as<int>(), toks.as<int>(), hid.as<float>(), anc0,
                       anc0 + (size_t)MBp * c.max_seq, score.as<float>(), c.mel_codes, c.hidden, rep_dev.as<float>(), c.max_seq,
                       mel_emb.as<float>(), mel_pos.as<float>(), c.max_mel_pos, Xd.as<float>(), B, pool_dev(), c.max_batch);
    MI_HIP(hipGetLastError());
}

void Gpt::pool_out_rows(const OutTable& tab, int n, int B, int32_t* tokens_dst, float* hidden_dst, float* score_dst) {
    MI_REQUIRE(n >= 0 && n <= GPT_MAX_BATCH && B >= 1 && B <= GPT_BEAM_MAX && pool_score.p, "gpt beam pool: retirement table");
    int rows = 1;                                                 // the score leaves in row 0's block
    for (int q = 0; q < n; ++q) {
        const OutSeg& g = tab.e[q];
        MI_REQUIRE(g.slot >= 0 && g.slot % B == 0 && g.slot + B <= cfg.max_batch && g.count >= 0 && g.count <= cfg.max_seq &&
                       g.sentence >= 0 && g.dst_row >= 0, "gpt beam pool: retirement entry");
        rows = std::max(rows, (int)g.count);
    }
    if (n == 0 || (!tokens_dst && !hidden_dst && !score_dst)) return;
    hipLaunchKernelGGL(gpt_pool_out_kernel, dim3(rows, n), dim3(256), 0, stream, tab, pool_dev(), toks.as<int>(), hid.as<float>(),
                       tokens_dst, hidden_dst, score_dst, B, cfg.max_seq, cfg.hidden, cfg.max_batch);
    MI_HIP(hipGetLastError());
}

}  // namespace mi
