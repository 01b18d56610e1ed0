// gpt_pool.h — what the engine and the C ABI see of pool-mode beam search (gpt_beam_pool.hip; include/mi355tts.h, "beam search
// with a finished pool").
#pragma once
#include "gpt.h"
#include "gpt_pick.h"

namespace mi {

constexpr int GPT_POOL_MAX_CAND = 64;            // K = (n_stop + 1) * num_beams candidates per selection, one wave sorts them

// the call's parameters on the device (read by the step kernel, so that a captured step does not depend on them)
struct GptPoolCfg { float length_penalty; int32_t early_stopping, sampling, pad; };

// words of a pool entry, per slot of the group: entry j of the pool (in pool order) is finished / holds PM_LEN tokens / lives in
// physical row PM_ROW of the group; PM_TOK is the last token of the entry in THIS physical row; PM_OPEN (first slot): `open`
enum { PM_FIN = 0, PM_LEN = 1, PM_ROW = 2, PM_TOK = 3, PM_OPEN = 4, GPT_POOL_META = 8 };

// the pool's device arrays, by slot
struct GptPoolDev {
    float* score;              // [slot]: pool scores in pool order
    int* meta;                 // [slot][GPT_POOL_META]
    int* anc;                  // [slot][max_seq]: the frozen ancestor list of physical row `slot` (positions 0 .. len - 2)
    float* hid;                // [slot][hidden]: its last last_hidden_state row
    unsigned* keys;            // [slot][codes]: scratch, the candidates' keys of one selection
    const GptPoolCfg* cfg;
    const GptSampleRec* recs;  // [slot]: the sentence's record at its group's first slot
};

// one selection of the unit entry
struct GptPoolSelect {
    int B, codes, n, max_new, n_stop;
    int stops[GS_WORDS - GS_STOP0];
    float length_penalty;
    int early_stopping, sampling;
    GptSampleRec rec;
};
// device arrays: logits / pen (B, codes), keys (B * codes) scratch, prev (B), pool_score / pool_fin (B) in / out, open_done (2:
// open in / out, done out), cand / cand_acc / cand_stop (K), parents / tokens / scores (B; -1 where no live candidate is left),
// pool_src (B: -1 - j = the entry that was at j, q >= 0 = candidate q)
void launch_gpt_pool_select(const float* logits, const float* pen, unsigned* keys, const GptPoolSelect& p, const float* prev,
                            float* pool_score, int32_t* pool_fin, int32_t* open_done, int32_t* cand, float* cand_acc,
                            int32_t* cand_stop, int32_t* parents, int32_t* tokens, float* scores, int32_t* pool_src, hipStream_t s);

}  // namespace mi
