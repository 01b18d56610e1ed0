"""CPU: the option table (csrc/options.h) through mi_set_option / mi_get_option — defaults, what each key does with an
out-of-range value, and the precedence default < environment (read once, at the first call) < mi_set_option.  Neither entry makes a
HIP call, so none of this needs a GPU.  Everything that changes an option runs in a child process: the options are process-wide
and the process running the suite keeps its own.

DEFAULTS below is the one deliberate second copy of the library's defaults: this is the test that pins them."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "text-to-speech-tts-onnx_amd")

DEFAULTS = {
    "gemm_big_tile_min": 160, "gemm_n192_min": 160, "gemm_mid_tile_min": 160, "gemm_dma3_k_min": 2048, "gemm_use_dma3": 1,
    "gemm_use_dma": 1, "gemm_big_tiles": 1, "gemm_n192": 1, "gemm_f32_dma": 1, "gemm_ring4": 1, "gemm_ring4_max": 256,
    "gemm_buf": 1, "gemm_f32_small": 1, "gemm_f32_small_max": 1024, "gemm_small16_max": 256, "gemm_row_split": 1,
    "gemm_sk": 1, "gemm_sk_stages": 0, "gemm_f32_x3": 1, "gemm_f32_x3p": 1, "gemm_f32_planes": 2, "gemm_f32_n64_pairs": 1,
    "gemm_f32_gconv": 1, "gemm_x3p_noalign": 0, "gemm_x3p_grid": 0, "gemm_x3d": 1, "gemm_x3d_min_eff": 90, "gemm_ph8": 1,
    "gemm_ph8_min_tiles": 200, "gemm_ph8_order": 1, "gemm_ph8_split_max": 2, "gemm_ph8_split_min_nk": 24,
    "gconv_two_taps": 1, "gconv16": 1,
    "attn_f32_x3": 2, "attn_f32_planes": 2, "attn_split": 2, "attn_xcd_map": 1, "attn_kv_planes": 1, "attn_lpt": 1,
    "attn_z_force": 0, "gpt_mfma_min": 9, "bigvgan_streams": 3,
    "aa_tile": 8192, "aa_pipe": 1, "aa_r": 16, "aaconv_lds_min": 0,
}
ON_OFF = ["gemm_use_dma3", "gemm_use_dma", "gemm_big_tiles", "gemm_n192", "gemm_f32_dma", "gemm_ring4", "gemm_buf",
          "gemm_f32_small", "gconv_two_taps", "gconv16", "attn_xcd_map", "attn_kv_planes", "attn_lpt", "aa_pipe"]       # store value != 0
CLAMP = {"attn_f32_x3": (0, 2), "attn_split": (0, 2), "attn_z_force": (0, 4), "bigvgan_streams": (1, 3), "gemm_ph8_split_max": (1, 4)}
REJECT = {"gemm_f32_planes": (2, 3), "attn_f32_planes": (2, 3)}
AS_GIVEN = sorted(set(DEFAULTS) - set(ON_OFF) - set(CLAMP) - set(REJECT))


def child(body: str, env: dict = None):
    """Runs `body` in a fresh interpreter (`_lib`, `json` imported; no MI355TTS_* variable but those in `env`) and returns the
    JSON document it prints last."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("MI355TTS_") or k == "MI355TTS_LIB"}
    e["MI355TTS_NO_TORCH"] = "1"                 # the loader's torch-first import is for processes that use the GPU
    e.update(env or {})
    code = f"import sys, json\nsys.path.insert(0, {PKG!r})\nfrom mi355tts import _lib\n{body}"
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_every_key_reports_its_default_in_a_fresh_process():
    got = child(f"print(json.dumps({{k: _lib.get_option(k) for k in {sorted(DEFAULTS)!r}}}))")
    assert got == DEFAULTS


def test_set_then_get_round_trips_under_each_keys_policy():
    body = f"""
out = {{}}
for k in {AS_GIVEN!r}:
    out[k] = []
    for v in (7, 0, -5, 1 << 40):
        _lib.set_option(k, v); out[k].append(_lib.get_option(k))
for k in {ON_OFF!r}:
    out[k] = []
    for v in (0, 1, 5, -1):
        _lib.set_option(k, v); out[k].append(_lib.get_option(k))
for k, (lo, hi) in {CLAMP!r}.items():
    out[k] = []
    for v in (lo - 1, lo, hi, hi + 1, 1 << 40, -(1 << 40)):
        _lib.set_option(k, v); out[k].append(_lib.get_option(k))
print(json.dumps(out))
"""
    got = child(body)
    for k in AS_GIVEN:
        assert got[k] == [7, 0, -5, 1 << 40], k
    for k in ON_OFF:
        assert got[k] == [0, 1, 1, 1], k
    for k, (lo, hi) in CLAMP.items():
        assert got[k] == [lo, lo, hi, hi, hi, lo], k


def test_rejecting_keys_fail_name_the_key_and_keep_the_value():
    body = f"""
out = {{}}
for k in {sorted(REJECT)!r}:
    _lib.set_option(k, 3)
    errs = []
    for v in (1, 4, 0, -2):
        try:
            _lib.set_option(k, v); errs.append(None)
        except _lib.MiError as e:
            errs.append(str(e))
    after = _lib.get_option(k)
    _lib.set_option(k, 2)
    out[k] = [errs, after, _lib.get_option(k)]
print(json.dumps(out))
"""
    got = child(body)
    for k in REJECT:
        errs, after, back = got[k]
        assert all(e is not None and k in e for e in errs), (k, errs)
        assert after == 3 and back == 2, k


def test_unknown_and_null_keys_fail_for_both_entries():
    body = """
import ctypes as C
L = _lib.load()
v = C.c_int64(-77)
out = {"set_unknown": L.mi_set_option(b"no_such_key", 1), "err_set": L.mi_last_error().decode(),
       "get_unknown": L.mi_get_option(b"no_such_key", C.byref(v)), "err_get": L.mi_last_error().decode(),
       "set_null": L.mi_set_option(None, 1), "get_null": L.mi_get_option(None, C.byref(v)),
       "get_null_value": L.mi_get_option(b"gemm_sk", None), "v": v.value,
       "env_only_has_no_key": L.mi_get_option(b"attn_z_max", C.byref(v))}
print(json.dumps(out))
"""
    got = child(body)
    for k in ("set_unknown", "get_unknown", "set_null", "get_null", "get_null_value", "env_only_has_no_key"):
        assert got[k] != 0, k
    assert "no_such_key" in got["err_set"] and "no_such_key" in got["err_get"]
    assert got["v"] == -77                                   # a failed get writes nothing


ENV = {"MI355TTS_X3D": "0", "MI355TTS_NO_DMA3_GEMM": "1", "MI355TTS_ATTN_X3": "9", "MI355TTS_GCONV16": "0"}
ENV_KEYS = ["gemm_x3d", "gemm_use_dma3", "attn_f32_x3", "gconv16"]


def test_environment_overrides_the_default():
    got = child(f"print(json.dumps([_lib.get_option(k) for k in {ENV_KEYS!r}]))", ENV)
    assert got == [0, 0, 2, 0]                               # MI355TTS_ATTN_X3=9 clamps to 2


def test_set_option_overrides_the_environment_and_stays():
    """The environment is read once, at the process's first call into the library — a later call (at the parent of this change:
    the first launch) never puts the variable's value back over a mi_set_option."""
    body = f"""
_lib.set_option("gemm_x3d", 1)
a = _lib.get_option("gemm_x3d")
_lib.set_option("gemm_sk", 2); _lib.load().mi_version()
print(json.dumps([a, _lib.get_option("gemm_x3d"), [_lib.get_option(k) for k in {ENV_KEYS[1:]!r}]]))
"""
    assert child(body, ENV) == [1, 1, [0, 2, 0]]


def test_environment_conventions():
    """'1' switches a MI355TTS_NO_* name off and nothing else does; '0' switches MI355TTS_GCONV* off and nothing else does; an
    integer variable of a rejecting key keeps the default when it is out of range."""
    keys = ["gemm_use_dma3", "gemm_buf", "gconv16", "gconv_two_taps", "gemm_f32_planes", "attn_f32_planes", "gemm_ph8_split_max", "attn_split"]
    env = {"MI355TTS_NO_DMA3_GEMM": "0", "MI355TTS_NO_BUF": "yes", "MI355TTS_GCONV16": "1", "MI355TTS_GCONV2": "off",
           "MI355TTS_F32_PLANES": "3", "MI355TTS_ATTN_PLANES": "7", "MI355TTS_PH8_SPLIT": "9", "MI355TTS_ATTN_NO_SPLIT": "1"}
    assert child(f"print(json.dumps([_lib.get_option(k) for k in {keys!r}]))", env) == [1, 1, 1, 1, 3, 2, 4, 0]


def _rows():
    src = open(os.path.join(PKG, "csrc", "options.h")).read()
    return re.findall(r'^\s*X\((\w+), ("\w+"|nullptr), ("\w+"|nullptr), (\w+), (-?\d+), (\w+), (-?\d+), (-?\d+)\)', src, flags=re.M)


def test_the_table_names_nothing_twice_and_matches_this_file():
    rows = _rows()
    assert len(rows) >= len(DEFAULTS)
    names = [r[0] for r in rows]
    keys = [r[1].strip('"') for r in rows if r[1] != "nullptr"]
    envs = [r[2].strip('"') for r in rows if r[2] != "nullptr"]
    assert len(set(names)) == len(names) and len(set(keys)) == len(keys) and len(set(envs)) == len(envs)
    assert all(r[1] != "nullptr" or r[2] != "nullptr" for r in rows)            # a row is reachable one way or the other
    assert {r[1].strip('"'): int(r[4]) for r in rows if r[1] != "nullptr"} == DEFAULTS
    policy = {r[1].strip('"'): (r[5], int(r[6]), int(r[7])) for r in rows if r[1] != "nullptr"}
    assert sorted(k for k, p in policy.items() if p[0] == "BOOL") == sorted(ON_OFF)
    assert {k: p[1:] for k, p in policy.items() if p[0] == "CLAMP"} == CLAMP
    assert {k: p[1:] for k, p in policy.items() if p[0] == "REJECT"} == REJECT
