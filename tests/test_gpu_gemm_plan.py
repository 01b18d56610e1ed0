"""GPU: every case of tests/golden/gemm_plan_census.json launches what the fixture recorded — the kernel label and the number of
launches, by the library profiler — on a device with the fixture's CU count.  (Grids: tests/test_gemm_plan.py, without a GPU.)"""
import json
import os

import pytest

from mi355tts import _lib

pytestmark = pytest.mark.gpu
FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_census.json")))


def test_device_has_the_fixtures_cu_count():
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count == FIX["cus"]


@pytest.mark.parametrize("case", FIX["cases"], ids=lambda c: "-".join(map(str, c["args"])))
def test_profiled_launch_matches_the_fixture(case):
    _lib.init(0)
    saved = {k: _lib.get_option(k) for k in case["options"]}
    _lib.prof_enable(("conv_gemm",))
    try:
        for k, v in case["options"].items():
            _lib.set_option(k, v)
        _lib.prof_reset()
        _lib.bench_conv_gemm(*case["args"], iters=1)
        got = sorted((k["kernel"], k["launches"]) for k in _lib.prof_kernels() if k["family"] == "conv_gemm" and k["launches"])
    finally:
        _lib.prof_enable(())
        for k, v in saved.items():
            _lib.set_option(k, v)
    assert got == sorted((l["label"], FIX["calls"]) for l in case["launches"]), got
