// options.hip — the option table's values, the one read of the environment, mi_set_option / mi_get_option by key (options.h).
#include "common.h"
#include <algorithm>
#include <cstdlib>
#include <mutex>

namespace mi {

enum EnvConv { ENV_INT, ENV_ONE_OFF, ENV_ZERO_OFF, ENV_ONE_ON, ENV_CUTS };
enum Policy { STORE, BOOL, CLAMP, REJECT };
struct Row { const char* key; const char* env; EnvConv conv; long dflt; Policy policy; long lo, hi; };
#define MI_OPT_ROW(name, key, env, conv, dflt, policy, lo, hi) {key, env, conv, dflt, policy, lo, hi},
static const Row kRows[OPT_COUNT] = {MI_OPTIONS(MI_OPT_ROW)};
#define MI_OPT_DEFAULT(name, key, env, conv, dflt, policy, lo, hi) {dflt},
std::atomic<long> g_opt[OPT_COUNT] = {MI_OPTIONS(MI_OPT_DEFAULT)};
static AttnCuts g_attn_cuts;
static std::atomic<long> g_option_epoch{0};

// the value a row stores for `v`; false: a REJECT row refuses it
static bool admit(const Row& r, long v, long* out) {
    *out = r.policy == BOOL ? v != 0 : r.policy == CLAMP ? std::min(std::max(v, r.lo), r.hi) : v;
    return r.policy != REJECT || (v >= r.lo && v <= r.hi);
}

void options_init() {
    static std::once_flag once;
    std::call_once(once, [] {
        for (int i = 0; i < OPT_COUNT; ++i) {
            const Row& r = kRows[i];
            const char* e = r.env ? std::getenv(r.env) : nullptr;
            if (!e) continue;
            long v = r.dflt;
            switch (r.conv) {
            case ENV_INT: if (!admit(r, std::atol(e), &v)) v = r.dflt; break;
            case ENV_ONE_OFF: if (e[0] == '1') v = 0; break;
            case ENV_ZERO_OFF: if (e[0] == '0') v = 0; break;
            case ENV_ONE_ON: if (e[0] == '1') v = 1; break;
            case ENV_CUTS: v = g_attn_cuts.n = std::max(0, std::sscanf(e, "%d,%d,%d", &g_attn_cuts.c[0], &g_attn_cuts.c[1], &g_attn_cuts.c[2])); break;
            }
            g_opt[i].store(v, std::memory_order_relaxed);
        }
    });
}

static int find_key(const char* key) {
    for (int i = 0; i < OPT_COUNT; ++i)
        if (kRows[i].key && std::strcmp(kRows[i].key, key) == 0) return i;
    return -1;
}

bool options_set(const char* key, long v) {
    const int i = find_key(key);
    if (i < 0) return false;
    long s;
    if (!admit(kRows[i], v, &s))
        throw Error(MI_EINVAL, std::string("mi_set_option: ") + key + " takes " + std::to_string(kRows[i].lo) + " .. " + std::to_string(kRows[i].hi));
    g_opt[i].store(s, std::memory_order_relaxed);
    return true;
}

bool options_get(const char* key, long* v) {
    const int i = find_key(key);
    if (i < 0) return false;
    *v = opt((Opt)i);
    return true;
}

const AttnCuts& opt_attn_cuts() { return g_attn_cuts; }

long env_int(const char* name, long dflt) { const char* e = std::getenv(name); return e ? std::atol(e) : dflt; }
bool env_first_is(const char* name, char c) { const char* e = std::getenv(name); return e && e[0] == c; }

long option_epoch() { return g_option_epoch.load(); }
void option_epoch_bump() { g_option_epoch.fetch_add(1); }
std::shared_mutex& option_lock() { static std::shared_mutex m; return m; }

}  // namespace mi
