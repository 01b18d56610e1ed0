// gpt_queue.hip — the sentence queue of the IndexTTS GPT (gpt_queue.h), and the host helpers capi.hip's generate entries share with it
#include "gpt_queue.h"

namespace mi {

void gpt_check_lengths(const GptCfg& c, int n, const int32_t* prompt_rows, const int32_t* max_new, int cap, const std::string& who) {
    for (int i = 0; i < n; ++i) {
        MI_REQUIRE(prompt_rows[i] >= 1 && max_new[i] >= 0 && max_new[i] <= cap, who + ": prompt_rows / max_new");
        MI_REQUIRE(max_new[i] == 0 || prompt_rows[i] + max_new[i] - 1 <= c.max_seq, who + ": prompt + max_new exceeds the KV cache (max_seq)");
        MI_REQUIRE(max_new[i] <= c.max_mel_pos, who + ": max_new exceeds the mel position table");
    }
}

std::vector<int32_t> gpt_fetch_stops(const int32_t* stop_ids, int n_stop, int mem, const std::string& who) {
    MI_REQUIRE(n_stop >= 0 && n_stop <= GS_WORDS - GS_STOP0 && (n_stop == 0 || stop_ids), who + ": at most 6 stop ids");
    std::vector<int32_t> stops(n_stop);
    if (n_stop) {
        if (mem == MI_HOST) std::copy(stop_ids, stop_ids + n_stop, stops.begin());
        else MI_HIP(hipMemcpy(stops.data(), stop_ids, (size_t)n_stop * 4, hipMemcpyDeviceToHost));
    }
    return stops;
}

std::vector<int32_t> gpt_state_words(const std::vector<int32_t>& stops, int penalty_range, int limit, bool done) {
    std::vector<int32_t> w(GS_WORDS, 0);
    w[GS_NSTOP] = (int32_t)stops.size(); w[GS_RANGE] = penalty_range; w[GS_UPDATE_PEN] = 1; w[GS_LIMIT] = limit;
    std::copy(stops.begin(), stops.end(), w.begin() + GS_STOP0);
    if (done) w[GS_DONE] = 1;
    return w;
}

void gpt_fill_penalty(Gpt& e, int rows, const float* src, hipMemcpyKind in_kind, int stride) {
    const int copies = stride == 1 ? 1 : rows;             // adjacent rows go in one copy
    const size_t n = e.cfg.mel_codes, len = (size_t)rows / copies * n;
    std::vector<float> ones;
    if (!src) ones.assign(len, 1.f);
    for (size_t r = 0; r < (size_t)copies; ++r) {
        float* dst = e.pen.as<float>() + r * stride * n;
        if (src) MI_HIP(hipMemcpyAsync(dst, src + r * len, len * 4, in_kind, e.stream));
        else MI_HIP(hipMemcpyAsync(dst, ones.data(), len * 4, hipMemcpyHostToDevice, e.stream));
    }
    if (!src) MI_HIP(hipStreamSynchronize(e.stream));      // `ones` is done with
}

bool gpt_read_states(Gpt& e, std::vector<int32_t>& all, int stride) {
    MI_HIP(hipMemcpyAsync(all.data(), e.state.p, all.size() * 4, hipMemcpyDeviceToHost, e.stream));
    MI_HIP(hipStreamSynchronize(e.stream));
    bool done = true;
    for (size_t b = 0; b < all.size() / GS_WORDS; b += stride) done &= all[b * GS_WORDS + GS_DONE] != 0;
    return done;
}

GptSampleRec gpt_sample_rec(float temperature, int top_k, float top_p, uint64_t seed) {
    MI_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "gpt sampling: temperature must be finite and > 0");
    MI_REQUIRE(top_k >= 0, "gpt sampling: top_k must be >= 0 (0 = every code)");
    MI_REQUIRE(std::isfinite(top_p) && top_p > 0.f && top_p <= 1.f, "gpt sampling: top_p must be in (0, 1]");
    GptSampleRec r{};
    r.inv_T = 1.0f / temperature; r.top_p = top_p; r.top_k = top_k;
    r.seed_lo = (uint32_t)seed; r.seed_hi = (uint32_t)(seed >> 32);
    return r;
}

// The driver's side is what the device states tell the engine: the prompt pass gives token 0, a unit is done when its sentence
// has produced lengths[i] tokens.  pass_of / unit_of name the pass and the unit that admitted each sentence (-1: max_new == 0);
// inside a pass the order is index order, so mi355tts.indextts.queue_schedule's (steps, passes) can be rebuilt from them.
void gpt_queue_schedule(int n, const int32_t* prompt_rows, const int32_t* max_new, const int32_t* lengths, int slots, int max_seq,
                        int beams, int32_t* steps, int32_t* n_passes, int32_t* pass_of, int32_t* unit_of) {
    const std::string who = "mi_gpt_queue_schedule";
    MI_REQUIRE(n >= 1 && n <= (1 << 20), who + ": n");
    MI_REQUIRE(prompt_rows && max_new && lengths && steps && n_passes && pass_of && unit_of, who + ": null argument");
    MI_REQUIRE(beams >= 1, who + ": beams must be >= 1");
    MI_REQUIRE(slots / beams >= 1, who + ": the slots must hold one unit");
    for (int i = 0; i < n; ++i)
        MI_REQUIRE(prompt_rows[i] >= 1 && max_new[i] >= 0 && lengths[i] >= 0 && lengths[i] <= max_new[i] && (max_new[i] == 0 || lengths[i] >= 1),
                   who + ": a sentence's rows, max_new and length");
    QueuePolicy pol;
    pol.start(n, prompt_rows, max_new, slots / beams, max_seq);
    std::vector<QueuePolicy::Entry> pass(pol.S);
    std::vector<int32_t> got(n, 0);                                  // tokens so far
    std::fill(pass_of, pass_of + n, -1);
    std::fill(unit_of, unit_of + n, -1);
    int64_t st = 0;
    int32_t np = 0;
    for (;;) {
        for (int k; (k = pol.form_pass(pass.data())) > 0; ++np)
            for (int j = 0; j < k; ++j) { pass_of[pass[j].sentence] = np; unit_of[pass[j].sentence] = pass[j].unit; got[pass[j].sentence] = 1; }
        for (int u = 0; u < pol.S; ++u)
            if (pol.owner[u] >= 0 && got[pol.owner[u]] >= lengths[pol.owner[u]]) pol.retire(u);
        if (pol.refill_due()) continue;
        if (pol.idle()) break;
        const int c = pol.run_length([&](int u) { return got[pol.owner[u]]; });
        MI_REQUIRE(c >= 1, who + ": a live unit is at its limit");
        st += c;
        for (int u = 0; u < pol.S; ++u)
            if (pol.owner[u] >= 0) got[pol.owner[u]] = std::min(lengths[pol.owner[u]], got[pol.owner[u]] + c);
    }
    MI_REQUIRE(st <= INT32_MAX, who + ": the step count does not fit 32 bits");
    *steps = (int32_t)st; *n_passes = np;
}

GptQueue::GptQueue(Gpt& g, const GptQueueArgs& a)
    : e(g), n(a.n), cap(a.cap), mem(a.mem), penalty_range(a.penalty_range), B(a.beam ? a.num_beams : 0), W(B ? B : 1),
      any_samp(a.temperature || a.top_k || a.top_p || a.seeds), per_round(a.per_round), pool_(a.beam && a.pool), prompts(a.prompts),
      tokens(a.tokens), hidden(a.hidden), scores(a.scores) {
    const GptCfg& c = e.cfg;
    const std::string who = a.who;
    if (a.beam) {                                                // mi_gpt_generate_beam's checks on num_beams
        MI_REQUIRE(B >= 1 && B <= GPT_BEAM_MAX, who + ": num_beams must be in [1, 8]");
        MI_REQUIRE(B <= c.mel_codes, who + ": num_beams exceeds the mel codes");
        MI_REQUIRE(B <= c.max_batch, who + ": num_beams exceeds the handle's max_batch");
    }
    if (pool_) {                                                 // mi_gpt_generate_beam_pool's checks on the search's parameters
        MI_REQUIRE(std::isfinite(a.length_penalty), who + ": length_penalty must be finite");
        MI_REQUIRE(a.early_stopping == 0 || a.early_stopping == 1, who + ": early_stopping must be 0 or 1");
    }
    MI_REQUIRE(n >= 1 && n <= (1 << 20), who + ": n");
    MI_REQUIRE(prompts && a.prompt_rows && a.max_new && cap >= 1, who + ": null argument");
    stops = gpt_fetch_stops(a.stop_ids, a.n_stop, mem, who);
    MI_REQUIRE(!any_samp || (a.temperature && a.top_k && a.top_p && a.seeds), who + ": the four sampling arrays come together or not at all");
    const int K = ((int)stops.size() + 1) * B;                   // pool mode: the candidates of a selection
    if (pool_) {
        MI_REQUIRE(K <= GPT_POOL_MAX_CAND && K <= c.mel_codes, who + ": (n_stop + 1) * num_beams must be <= 64 and <= mel_codes");
        MI_REQUIRE(!any_samp || c.mel_codes <= GPT_SAMPLE_MAX_CODES, who + ": sampling supports at most 16384 mel codes");
    }
    gpt_check_lengths(c, n, a.prompt_rows, a.max_new, cap, who);
    row0.resize(n);
    size_t rows_total = 0;
    for (int i = 0; i < n; ++i) { row0[i] = rows_total; rows_total += (size_t)a.prompt_rows[i]; }
    GptModeScope mode(e, any_samp && !pool_);                    // (checks that the handle can sample)
    recs.resize(any_samp ? n : 0);
    for (int i = 0; i < (int)recs.size(); ++i) {
        recs[i] = gpt_sample_rec(a.temperature[i], a.top_k[i], a.top_p[i], a.seeds[i]);
        MI_REQUIRE(!pool_ || a.top_k[i] == 0 || a.top_k[i] >= K, who + ": top_k must be 0 or at least (n_stop + 1) * num_beams");
    }
    e.set_rep_value(a.repeat_value);
    pol.start(n, a.prompt_rows, a.max_new, c.max_batch / W, c.max_seq);
    if (pool_) {
        e.pool_ensure();
        e.pool_set_cfg(GptPoolCfg{a.length_penalty, a.early_stopping, any_samp ? 1 : 0, 0});
        meta.assign((size_t)pol.S * W * GPT_POOL_META, 0);
        // a sentence with max_new == 0 takes no group: its score is 0 from the start
        for (int i = 0; i < n && scores; ++i) {
            if (a.max_new[i] != 0) continue;
            if (mem == MI_HOST) scores[i] = 0.f;
            else MI_HIP(hipMemsetAsync(scores + i, 0, 4, e.stream));
        }
    } else if (B) e.beam_ensure();
    // every slot the decode steps will run over starts as a finished one: a slot no sentence ever takes is a no-op
    all.assign((size_t)pol.S * W * GS_WORDS, 0);
    for (int b = 0; b < pol.S * W; ++b) all[(size_t)b * GS_WORDS + GS_DONE] = 1;
    MI_HIP(hipMemcpyAsync(e.state.p, all.data(), all.size() * 4, hipMemcpyHostToDevice, e.stream));
    MI_HIP(hipStreamSynchronize(e.stream));
    n_out.assign(n, 0); copied.assign(n, 0); retired.assign(n, 0);
}

// rows [first, first + count) of sentence i, held by `slot` (beams: its group's first slot, noted once and whole), join the table
void GptQueue::note(int slot, int i, int first, int count) {
    if (count <= 0) return;
    MI_REQUIRE(n_tab < GPT_MAX_BATCH, "gpt queue: copy-out table overflow");
    Gpt::OutSeg& g = tab.e[n_tab++];
    g.slot = slot; g.first = first; g.count = count; g.sentence = i;
    g.dst_row = (int64_t)i * cap + first;
    copied[i] = first + count;
}

// The table's rows leave in one launch (beams: hypothesis 0's tokens and rows along its ancestors, and its score; pool mode:
// pool entry 0's along its frozen list).  MI_DEVICE: straight into the caller's arrays.  MI_HOST: packed into the staging buffers,
// one device-to-host copy per array, then placed by the host.
void GptQueue::flush() {
    if (n_tab == 0) return;
    const int h = e.cfg.hidden;
    auto launch = [&](const Gpt::OutTable& t, int32_t* tok, float* hid, float* sc) {
        if (pool_) e.pool_out_rows(t, n_tab, B, tok, hid, sc);
        else if (B) e.beam_out_rows(t, n_tab, B, tok, hid, sc);
        else e.copy_out_rows(t, n_tab, tok, hid);
    };
    if (mem == MI_DEVICE) {
        launch(tab, tokens, hidden, scores);
    } else {
        Gpt::OutTable packed = tab;
        size_t rows = 0;
        for (int k = 0; k < n_tab; ++k) {
            packed.e[k].dst_row = (int64_t)rows;
            if (B) packed.e[k].sentence = k;                     // the staged score's place
            rows += (size_t)tab.e[k].count;
        }
        e.io_a.ensure(rows * 4); e.io_b.ensure(rows * h * 4);
        h_tok.resize(rows); h_hid.resize(rows * h);
        if (B) { e.io_s.ensure((size_t)n_tab * 4); h_sc.resize(n_tab); }
        launch(packed, tokens ? e.io_a.as<int32_t>() : nullptr, hidden ? e.io_b.as<float>() : nullptr, scores ? e.io_s.as<float>() : nullptr);
        if (tokens && rows) MI_HIP(hipMemcpyAsync(h_tok.data(), e.io_a.p, rows * 4, hipMemcpyDeviceToHost, e.stream));
        if (hidden && rows) MI_HIP(hipMemcpyAsync(h_hid.data(), e.io_b.p, rows * h * 4, hipMemcpyDeviceToHost, e.stream));
        if (scores) MI_HIP(hipMemcpyAsync(h_sc.data(), e.io_s.p, (size_t)n_tab * 4, hipMemcpyDeviceToHost, e.stream));
        MI_HIP(hipStreamSynchronize(e.stream));
        for (int k = 0; k < n_tab; ++k) {
            const Gpt::OutSeg& g = tab.e[k];
            const size_t src = (size_t)packed.e[k].dst_row, dst = (size_t)g.dst_row;
            if (tokens) std::memcpy(tokens + dst, h_tok.data() + src, (size_t)g.count * 4);
            if (hidden) std::memcpy(hidden + dst * h, h_hid.data() + src * h, (size_t)g.count * h * 4);
            if (scores) scores[g.sentence] = h_sc[k];             // (beams only: a greedy queue has no scores)
        }
    }
    n_tab = 0;
}

// A sentence enters a unit: its W slots get the state words, the first one a penalty row of ones and, in a sampled queue, the record.
// beams: the B slots of a refilled group get the sentence's state words, the group's first slot its side-0 penalty row of ones
// (selection 0 reads side 0: GS_NDEC = 0), both in stream order behind the retirement launch of the tenant before.  Nothing
// else of that tenant can be read (checked against gpt_beam.hip):
//   - ancestor tables: selection n copies entries [0, nprev = n) from the side it reads and writes entry n, so from nprev = 0
//     on every entry below n of the side in use was written by this sentence; attention, the reset lookup and retirement read
//     entries below GS_NDEC only;
//   - scores: selection 0 (`first`) starts every candidate from 0 and never adds the scores it loaded;
//   - penalties: selection 0 reads the first slot's side-0 row alone (parent 0) and writes all B rows of side 1; selection 1
//     reads those and writes all B rows of side 0: side 1, and rows 1 .. B-1 of side 0, are written before they are read;
//   - toks / hid: selection n writes row n of every slot of the group before GS_NDEC becomes n + 1, and every read is of a
//     row below GS_NDEC, so a stale row lies at an index >= ndec;
//   - the KV cache: the pass rewrites the prompt's rows in the first slot, a decode step writes position P + n - 1 of its own
//     slot before its attention reads it, and no key at or beyond the history is visited.
// pool mode: the group's pool is made empty as well (Gpt::pool_reset_group: what pool_begin sets for every slot of a call, for
// this group's B slots), in the same stream order: scores -1e9, every meta word 0 except PM_ROW = the slot's index in the group
// and PM_OPEN = 1, and the sentence's sampling record.  The selection loads PM_FIN / PM_LEN / PM_ROW / PM_OPEN and the scores of
// all B entries before it writes any, so these are reset; PM_LEN and PM_TOK go to 0 with them although no stale value of either
// could reach a result (an entry's PM_LEN is used only when its PM_FIN is set, and both are written together when a candidate
// enters).  What is not reset, and the write that precedes every read (checked against gpt_beam_pool.hip):
//   - pool_anc: a candidate entering the pool at selection n writes entries [0, n) of its physical row and gets PM_LEN = n + 1;
//     retirement reads entries below PM_LEN - 1 of the row of an entry whose PM_FIN is set, i.e. one this sentence froze; the
//     selection itself never reads pool_anc;
//   - pool_hid, PM_TOK: written whole for the physical row in that same freeze, read by retirement alone, for that row;
//   - a physical row is reused only for an entry that left the pool: rows of kept entries are marked used before a free one
//     is taken, and PM_ROW starts as the identity, so two entries never share a row;
//   - pool_keys: scratch of one selection, every word [0, R * codes) it reads is written earlier in that selection;
//   - PM_LEN: as above; PM_FIN = 0 until this sentence's own candidate sets both.
void GptQueue::admit(int unit, int i) {
    const int slot = unit * W;
    const std::vector<int32_t> w = gpt_state_words(stops, penalty_range, pol.max_new[i], false);
    std::vector<int32_t> ws((size_t)W * GS_WORDS);
    for (int b = 0; b < W; ++b) std::copy(w.begin(), w.end(), ws.begin() + (size_t)b * GS_WORDS);
    MI_REQUIRE(slot >= 0 && slot + W <= e.cfg.max_batch, "gpt queue: unit slot");
    MI_HIP(hipMemcpyAsync(e.state.as<int32_t>() + (size_t)slot * GS_WORDS, ws.data(), ws.size() * 4, hipMemcpyHostToDevice, e.stream));
    MI_HIP(hipStreamSynchronize(e.stream));                      // `ws` is done with
    if (!B && slot == 0) e.history = 0;                          // as Gpt::set_state did for the greedy queue alone; settle() writes it for both
    e.reset_penalty(slot);
    if (pool_) e.pool_reset_group(unit, B, any_samp ? &recs[i] : nullptr);
    else if (any_samp) e.set_sampling_slot(&recs[i], slot);
}

int GptQueue::pool_len(int unit) const {
    const int32_t* mw = meta.data() + (size_t)unit * W * GPT_POOL_META;
    return mw[PM_FIN] ? std::min(std::max(mw[PM_LEN], 0), std::min(cap, e.cfg.max_seq)) : 0;
}

void GptQueue::read_states() {
    if (pool_) MI_HIP(hipMemcpyAsync(meta.data(), e.pool_meta.p, meta.size() * 4, hipMemcpyDeviceToHost, e.stream));
    gpt_read_states(e, all);                                     // (synchronises the stream: both copies have landed)
}

bool GptQueue::round() {
    const GptCfg& c = e.cfg;
    hipStream_t s = e.stream;
    const hipMemcpyKind in = mem == MI_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    for (;;) {
        // 1. admit: the passes the policy forms, each sentence's prompt packed behind the one before
        QueuePolicy::Entry pass[GPT_MAX_BATCH];
        bool ran = false;
        for (int k; (k = pol.form_pass(pass)) > 0; ran = true) {
            Gpt::Seg segs[GPT_MAX_BATCH];
            for (int j = 0; j < k; ++j) {
                const int i = pass[j].sentence, rows = pol.prompt_rows[i], first = pass[j].first;
                admit(pass[j].unit, i);
                MI_HIP(hipMemcpyAsync(e.X.as<float>() + (size_t)first * c.hidden, prompts + row0[i] * c.hidden, (size_t)rows * c.hidden * 4, in, s));
                segs[j].first = first; segs[j].rows = rows; segs[j].slot = pass[j].unit * W; segs[j].pad = 0;
            }
            e.forward_packed(segs, k);
            ++passes;
        }
        if (ran) read_states();
        // 2. retire every finished unit: its tokens and rows go out, the unit is free
        for (int u = 0; u < pol.S; ++u) {
            const int i = pol.owner[u], b = u * W;
            if (i < 0 || !word(u, GS_DONE)) continue;
            const int nt = n_out[i] = pool_ ? pool_len(u) : held(u);   // pool mode: entry 0's length, not the selections run
            if (B || per_round) {
                note(b, i, copied[i], nt - copied[i]);
            } else {                                             // the blocking greedy entry: one copy per array per sentence, no table kernel
                copy_out(tokens ? tokens + (size_t)i * cap : nullptr, e.toks.as<int32_t>() + (size_t)b * c.max_seq, (size_t)nt * 4, mem, s);
                copy_out(hidden ? hidden + (size_t)i * cap * c.hidden : nullptr, e.hid.as<float>() + (size_t)b * c.max_seq * c.hidden,
                         (size_t)nt * c.hidden * 4, mem, s);
            }
            retired[i] = 1;
            pol.retire(u);
        }
        flush();                                                 // in stream order before a pass can refill the units
        if (pol.refill_due()) continue;
        // 3. finish, or decode as far as the policy says and look again
        if (pol.idle()) { ended_ = true; return false; }
        const int cs = pol.run_length([&](int u) { return word(u, GS_NDEC); });
        MI_REQUIRE(cs >= 1, "gpt queue: a live slot is at its limit");
        if (pool_) e.decode_pool_steps(pol.S, B, cs);
        else if (B) e.decode_beam_steps(pol.S, B, cs);
        else e.decode_batch_steps(pol.S, cs);
        steps += cs;
        read_states();
        return true;
    }
}

// With beams nothing leaves here: no row of a live group is final, the whole sentence leaves when its group is retired.
void GptQueue::publish_live() {
    if (B) return;
    for (int u = 0; u < pol.S; ++u)
        if (pol.owner[u] >= 0) note(u, pol.owner[u], copied[pol.owner[u]], held(u) - copied[pol.owner[u]]);
    flush();
}

void GptQueue::settle() {
    e.history = all[GS_HIST];
    MI_HIP(hipStreamSynchronize(e.stream));
}

void GptQueue::report(int32_t* count, int32_t* done, int32_t* finished, int32_t* stats) const {
    bool fin = !pol.waiting();
    for (int i = 0; i < n; ++i) {
        count[i] = n_out[i];
        if (done) done[i] = retired[i] || pol.max_new[i] == 0;
    }
    for (int u = 0; u < pol.S; ++u) {
        const int i = pol.owner[u];
        if (i < 0) continue;
        // beams: a finished group is done for the caller once it has been retired (count = n_out)
        const int32_t d = B ? 0 : word(u, GS_DONE) != 0;
        count[i] = copied[i];
        if (done) done[i] = d;
        fin = fin && d;
    }
    if (finished) *finished = fin ? 1 : 0;
    if (stats) { stats[0] = (int32_t)steps; stats[1] = (int32_t)passes; }
}

}  // namespace mi
