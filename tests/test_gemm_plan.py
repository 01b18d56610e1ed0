"""CPU: gemm_plan (csrc/gemm_conv.hip), the one decision behind launch_conv_gemm, asked through the host-only entry
mi_conv_gemm_plan and held against tests/golden/gemm_plan_census.json: the launches (kernel label from the library profiler,
grid and block from a kernel trace) that the build BEFORE the plan existed made for tools/gemm_plan_census.py's cases on an
MI355X.  The GPU half is tests/test_gpu_gemm_plan.py."""
import json
import os
import re

import pytest

from mi355tts import _lib

FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_census.json")))


def plan_of(case, cus):
    saved = {k: _lib.get_option(k) for k in case["options"]}
    try:
        for k, v in case["options"].items():
            _lib.set_option(k, v)
        return _lib.conv_gemm_plan(*case["args"], cus=cus)
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)


@pytest.fixture(scope="module")
def plans():
    return [plan_of(c, FIX["cus"]) for c in FIX["cases"]]


def test_launch_counts_and_grids_are_the_recorded_ones(plans):
    assert len(FIX["cases"]) >= 20 and any(len(c["launches"]) == 2 for c in FIX["cases"])
    for c, pl in zip(FIX["cases"], plans):
        assert len(pl) == len(c["launches"]), (c["args"], pl)
        for p, l in zip(pl, c["launches"]):
            assert p["grid"] == l["grid"], (c["args"], p, l)


def test_each_kind_has_one_label_form(plans):
    """Apart from the type names (and stream-K's ring depth, which its launcher takes from the type: 2 stages for 16-bit, 3 for
    fp32), and from the epilogue switch (the LDS-staged or the direct instantiation of the same kind, which the plan reports as
    lds_epi), a kind is one launch statement: one label.  And no two kinds share one."""
    form_of, spelled = {}, set()
    for c, pl in zip(FIX["cases"], plans):
        for p, l in zip(pl, c["launches"]):
            form = re.sub(r"\b(_Float16|__bf16|float)\b", "T", l["label"])
            form = re.sub(r"^(linear_sk_kernel<T, T, \w+), [23]>$", r"\1, stages>", form)
            assert form_of.setdefault((p["kind"], p["lds_epi"]), form) == form, (c["args"], p, l)
            # where the label spells the epilogue switch (the DMA kernels, stream-K, x3), the plan's lds_epi is that argument
            m = re.match(r"(?:conv_gemm_dma_kernel<T, T|linear_sk_kernel<T, T|linear_x3_kernel<T), (true|false)\b", form)
            if m:
                assert p["lds_epi"] == (m.group(1) == "true"), (c["args"], p, l)
                spelled.add(p["kind"])
    assert spelled == {"dma 64x64", "dma 64x64 fp16 pairs", "dma 128", "dma 128 ring4", "stream-k", "x3"}, spelled
    kinds = {k for k, _ in form_of}
    assert kinds == set(_lib.GEMM_KINDS[1:]), set(_lib.GEMM_KINDS[1:]) - kinds
    by_form = {}
    for (kind, _), form in form_of.items():
        assert by_form.setdefault(form, kind) == kind, (form, kind, by_form[form])


def test_the_row_split_plans_its_rest_as_a_problem_of_its_own(plans):
    c = next(i for i, c in enumerate(FIX["cases"]) if len(c["launches"]) == 2)
    a, b = plans[c]
    assert a["kind"] == "ph8" and a["Tm"] * 256 < FIX["cases"][c]["args"][2] and b["kind"].startswith("dma ")
    # ... and a device with other CUs plans other rounds: the split follows `cus`, not a constant
    assert len(plan_of(FIX["cases"][c], 304)) == 1


@pytest.mark.parametrize("B, T", [(8, 2252), (2, 9008), (4, 4504)])
def test_a_batch_is_planned_as_the_rows_the_launch_flattens_it_to(B, T):
    """launch_conv_gemm makes one M axis of a one-tap batch over contiguous items before it plans; so does the entry: 18016 rows in
    B items give the plan of the recorded B = 1 case, row split included."""
    c = next(c for c in FIX["cases"] if len(c["launches"]) == 2)
    dt, _, rows, Cin, N, taps = c["args"]
    assert B * T == rows
    got = _lib.conv_gemm_plan(dt, B, T, Cin, N, taps, cus=FIX["cus"])
    assert got == plan_of(c, FIX["cus"])
    assert [p["grid"] for p in got] == [l["grid"] for l in c["launches"]]
    # seven taps keep the items apart (B stays in the grid): nothing to flatten, nothing to split
    conv = _lib.conv_gemm_plan(dt, B, T, 512, N, 7, cus=FIX["cus"])
    assert len(conv) == 1 and all(v >= 0 for p in conv for v in p["grid"])


def test_bad_arguments_are_refused():
    L = _lib.load()
    import ctypes as C
    out, n = (C.c_int32 * 20)(), C.c_int(0)
    good = [_lib.MI_F16, 1, 300, 64, 32, 7, 1, 0, 256]
    assert L.mi_conv_gemm_plan(*good, out, C.byref(n)) == 0 and n.value == 1
    for i, v in ((0, 7), (1, 0), (2, 0), (3, 0), (4, -1), (5, 0), (6, 0), (8, 0)):
        bad = list(good)
        bad[i] = v
        assert L.mi_conv_gemm_plan(*bad, out, C.byref(n)) == _lib.MI_EINVAL, bad
    assert L.mi_conv_gemm_plan(*good, None, C.byref(n)) == _lib.MI_EINVAL
    assert L.mi_conv_gemm_plan(*good, out, None) == _lib.MI_EINVAL
