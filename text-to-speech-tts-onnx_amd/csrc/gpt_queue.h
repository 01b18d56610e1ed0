// gpt_queue.h — the IndexTTS GPT's sentence queue (include/mi355tts.h, "sentence queue"): n sentences through S = min(max_batch,
// n) slots, a slot refilled as soon as its sentence stops, every prompt pass packed (Gpt::forward_packed).  QueuePolicy decides,
// GptQueue launches, the C-ABI entries (capi.hip) drive it; and what the queue shares with capi.hip's other generate entries.
#pragma once
#include "gpt.h"
#include "gpt_pick.h"
#include "gpt_pool.h"
#include <algorithm>

namespace mi {

// what the generate entries share -----------------------------------------------------------------------------------------
// per-sentence lengths against the caller's row capacity, the KV cache and the mel position table
void gpt_check_lengths(const GptCfg& c, int n, const int32_t* prompt_rows, const int32_t* max_new, int cap, const std::string& who);
// the stop ids on the host, from the host or the device
std::vector<int32_t> gpt_fetch_stops(const int32_t* stop_ids, int n_stop, int mem, const std::string& who);
// the state words of a sentence about to start: limit = its max_new (0: none), done = it generates nothing
std::vector<int32_t> gpt_state_words(const std::vector<int32_t>& stops, int penalty_range, int limit, bool done);
// penalty rows := the caller's `rows` vectors, or ones; row r goes to slot r * stride (beam search: a group's first slot)
void gpt_fill_penalty(Gpt& e, int rows, const float* src, hipMemcpyKind in_kind, int stride = 1);
// the state words of slots 0 .. all.size() / GS_WORDS - 1 -> all; true when every stride-th slot is done
bool gpt_read_states(Gpt& e, std::vector<int32_t>& all, int stride = 1);
// one sentence's parameters, validated -> the device record
GptSampleRec gpt_sample_rec(float temperature, int top_k, float top_p, uint64_t seed);

// the calls that follow on the handle choose tokens by sampling (off: greedy); greedy again when the scope ends.  With `recs`
// the records of slots 0 .. nb-1 are uploaded as well (null: greedy); the queue uploads a slot's record when it admits a sentence.
struct GptModeScope {
    Gpt& e;
    GptModeScope(Gpt& g, bool on) : e(g) {
        if (on) MI_REQUIRE(e.cfg.mel_codes <= GPT_SAMPLE_MAX_CODES, "gpt: sampling supports at most 16384 mel codes");
        e.sampled = on ? 1 : 0;
    }
    GptModeScope(Gpt& g, const GptSampleRec* recs, int nb) : GptModeScope(g, recs != nullptr) {
        if (recs) e.set_sampling(recs, nb);
    }
    ~GptModeScope() { e.sampled = 0; }
};

// the handle runs beam groups (forward_rows / forward_packed leave the token choice to selection 0; pool: to the pool-mode
// selection 0) until the scope ends
struct GptBeamScope {
    Gpt& e;
    GptBeamScope(Gpt& g, int B, bool pool = false) : e(g) { e.beams = B; e.pool = B && pool ? 1 : 0; }
    ~GptBeamScope() { e.beams = 0; e.pool = 0; }
};

// Steps 1-3 of the header's scheduling policy, decided here and nowhere else.  Plain host code: no HIP call, no Gpt.  A unit is a slot,
// or with beams a group of B slots.  The driver (GptQueue::round; gpt_queue_schedule) reports the units done and the tokens they hold.
struct QueuePolicy {
    std::vector<int32_t> prompt_rows, max_new;
    std::vector<int> owner;              // the sentence in each unit, -1 = free
    int S = 0, max_seq = 0;              // units; the packed rows a pass may hold
    int next = 0, live = 0;              // the next waiting sentence; units in use
    bool freed = false;                  // a unit was retired since refill_due() was asked last

    struct Entry { int sentence, unit, first; };     // `first`: the sentence's first packed row of the pass

    void start(int n, const int32_t* rows, const int32_t* limits, int units, int max_seq_) {
        prompt_rows.assign(rows, rows + n); max_new.assign(limits, limits + n);
        S = std::min(units, n); max_seq = max_seq_;
        owner.assign(S, -1);
        next = 0; live = 0; freed = false;
        skip_empty();
    }
    int n() const { return (int)max_new.size(); }
    bool waiting() const { return next < n(); }
    bool idle() const { return live == 0; }
    // 1. the next pass -> out (room for S entries), in index order, each sentence into the lowest free unit; 0: nothing to admit
    int form_pass(Entry* out) {
        int k = 0, total = 0;
        while (live < S && waiting()) {
            const int rows = prompt_rows[next];
            if (k > 0 && total + rows > max_seq) break;             // the first sentence of a pass always fits
            int unit = 0;
            while (owner[unit] >= 0) ++unit;
            owner[unit] = next; ++live;
            out[k++] = {next, unit, total};
            total += rows;
            ++next;
            skip_empty();
        }
        return k;
    }
    // 2. the driver found the unit's sentence done
    void retire(int unit) { owner[unit] = -1; --live; freed = true; }
    // ... and when it has retired all it found: true = a unit came free and a sentence waits, so step 1 before any decode step
    bool refill_due() { const bool r = freed && waiting(); freed = false; return r; }
    // 3. decode steps up to the nearest limit of a live unit, at most 16; tokens(unit) = what its sentence holds so far
    template <typename F> int run_length(F&& tokens) const {
        int c = 16;
        for (int u = 0; u < S; ++u)
            if (owner[u] >= 0) c = std::min(c, max_new[owner[u]] - (int)tokens(u));
        return c;
    }
    void skip_empty() { while (waiting() && max_new[next] == 0) ++next; }        // max_new == 0 takes no unit
};

// mi_gpt_queue_schedule: the policy driven on the host by the lengths the sentences will have
void gpt_queue_schedule(int n, const int32_t* prompt_rows, const int32_t* max_new, const int32_t* lengths, int slots, int max_seq,
                        int beams, int32_t* steps, int32_t* n_passes, int32_t* pass_of, int32_t* unit_of);

// the arguments of the queue entries, in the C ABI's order; prompts, tokens, hidden and scores stay the caller's until the queue goes
struct GptQueueArgs {
    const char* who = "";                // the entry's name, for messages
    int n = 0;
    const float* prompts = nullptr;
    const int32_t *prompt_rows = nullptr, *max_new = nullptr, *stop_ids = nullptr;
    int n_stop = 0;
    float repeat_value = 0.f;
    int penalty_range = 0;
    int32_t* tokens = nullptr;
    float* hidden = nullptr;
    int cap = 0, mem = MI_HOST;
    const float* temperature = nullptr;  // the four sampling arrays, or none
    const int32_t* top_k = nullptr;
    const float* top_p = nullptr;
    const uint64_t* seeds = nullptr;
    bool beam = false;                   // the "_beam" entries: num_beams hypotheses per sentence, their scores (n) or null
    int num_beams = 0;
    float* scores = nullptr;
    bool pool = false;                   // the "_beam_pool" entries: pool mode (the sampling arrays then belong to the beam sampling)
    float length_penalty = 0.f;
    int early_stopping = 0;
    bool per_round = false;              // sessions: tokens and rows leave after every round; blocking entry: at retirement only
};

// The loop of a session (mi_gpt_queue_begin / _advance / _end), which stops after every run of decode steps; the blocking entry is a
// session driven to its end inside one call.  With beams (B != 0) the unit of the schedule is a group, B consecutive slots: group g =
// slots gB .. gB + B - 1, S = min(max_batch / B, n) groups.  B == 0 launches exactly what the queue launched before groups existed.
// Pool mode (B != 0 and `pool`): the groups run the pool-mode selection (gpt_beam_pool.hip); GS_NDEC counts the selections run,
// which is what max_new bounds and the policy reads, and a sentence's length is PM_LEN of its group's pool entry 0.
class GptQueue {
public:
    // validation (all of it before anything is launched) and the start state: every slot finished, nothing admitted
    GptQueue(Gpt& e, const GptQueueArgs& a);
    // one round of the policy: admit and retire until nothing more can be admitted, then one run of c <= 16 decode steps and a look
    // at the states; false when there was nothing left to decode (the queue has ended)
    bool round();
    // sessions, after a round: everything the live slots hold by now leaves, finished ones included (the next round retires them)
    void publish_live();
    // count / done / finished as mi_gpt_queue_advance defines them (done and finished may be null), stats = {steps, passes} or null
    void report(int32_t* count, int32_t* done, int32_t* finished, int32_t* stats) const;
    // the end of an entry that ran rounds: the host mirror of slot 0's history, and the stream drained
    void settle();
    bool ended() const { return ended_; }
    bool sampled() const { return any_samp && !pool_; }          // pool mode draws inside its selection, not with the sampler
    int beams() const { return B; }
    bool pool() const { return pool_; }

private:
    Gpt& e;
    QueuePolicy pol;
    int n, cap, mem, penalty_range, B, W;        // B: beams per sentence (0 = no beam search); W: slots per unit
    bool any_samp, per_round, pool_, ended_ = false;
    const float* prompts;
    int32_t* tokens;
    float *hidden, *scores;              // scores: beams only, the caller's (n) or null
    std::vector<int32_t> stops, all, n_out, copied, meta;      // meta: pool mode, the pool words of slots 0 .. S * W - 1
    std::vector<GptSampleRec> recs;
    std::vector<size_t> row0;
    std::vector<char> retired;
    long steps = 0, passes = 0;
    Gpt::OutTable tab; int n_tab = 0;    // the copy-out entries gathered since the last launch
    std::vector<int32_t> h_tok;          // MI_HOST: what the copy-out kernel packed, on the host
    std::vector<float> h_hid, h_sc;

    int32_t word(int unit, int w) const { return all[(size_t)unit * W * GS_WORDS + w]; }     // of the unit's first slot
    int held(int unit) const { return std::min(word(unit, GS_NDEC), pol.max_new[pol.owner[unit]]); }
    int pool_len(int unit) const;        // pool mode: the tokens pool entry 0 of the unit holds (0: no finished entry)
    void read_states();                  // the state words (pool mode: and the pool words) of the slots in use -> all (, meta)
    void admit(int unit, int sentence);
    void note(int slot, int sentence, int first, int count);
    void flush();
};

}  // namespace mi
