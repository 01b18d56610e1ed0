"""CPU: tools/boundary_gaps.py on a hand-written kernel trace of twelve dispatches with known gaps — one overlapping pair (a
negative gap), one kernel that is last in the file (no gap, no period), rows out of time order."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "boundary_gaps.py")

A = "void mi::linear_x3d_kernel<192, true, 1>(mi::ConvGemmDev)"
B = "void mi::attn_x3f_kernel<false, true, true>(mi::AttnArgs)"
C = "void mi::linear_x3d_kernel<64, true, 3>(mi::ConvGemmDev)"
D = "tail_kernel(int)"
SA, SB, SC, SD = "linear_x3d_kernel<192, true, 1>", "attn_x3f_kernel<false, true, true>", "linear_x3d_kernel<64, true, 3>", "tail_kernel"

# (kernel, start ns, end ns): A B C A B C A B C A C D
DISPATCHES = [
    (A, 1000, 51000),       # gap 2000
    (B, 53000, 99000),      # gap 1000
    (C, 100000, 125000),    # gap 3000
    (A, 128000, 180000),    # gap 1000
    (B, 181000, 229000),    # the next starts before this ends: gap -1000
    (C, 228000, 252000),    # gap 4000
    (A, 256000, 304000),    # gap 3000
    (B, 307000, 351000),    # gap 2000
    (C, 353000, 379000),    # gap 2000
    (A, 381000, 431000),    # gap 6000, followed by C
    (C, 437000, 462000),    # gap 1000
    (D, 463000, 470000),    # last: no gap
]
HEADER = ('"Kind","Agent_Id","Queue_Id","Stream_Id","Thread_Id","Dispatch_Id","Kernel_Id","Kernel_Name","Correlation_Id",'
          '"Start_Timestamp","End_Timestamp","LDS_Block_Size","Scratch_Size","VGPR_Count","Accum_VGPR_Count","SGPR_Count",'
          '"Workgroup_Size_X","Workgroup_Size_Y","Workgroup_Size_Z","Grid_Size_X","Grid_Size_Y","Grid_Size_Z"')


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("boundary_gaps", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    path = tmp_path_factory.mktemp("trace") / "x_kernel_trace.csv"
    order = [7, 0, 3, 11, 1, 2, 5, 4, 6, 10, 9, 8]           # the file is not in time order
    lines = [HEADER]
    for i in order:
        k, s, e = DISPATCHES[i]
        lines.append(f'"KERNEL_DISPATCH","Agent 2",1,20,263,{i + 1},{ord(k[-2])},"{k}",{i + 1},{s},{e},161280,0,68,0,112,768,1,1,196608,1,1')
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_short_names(tool):
    assert [tool.short_name(k) for k in (A, B, C, D)] == [SA, SB, SC, SD]
    assert tool.short_name("void f<(anonymous namespace)::g(int)>(float*)") == "f<(anonymous namespace)::g(int)>"


def test_by_kernel(tool, trace):
    by_k, _ = tool.analyse(tool.read_trace(trace))
    assert set(by_k) == {SA, SB, SC, SD}
    a, b, c, d = by_k[SA], by_k[SB], by_k[SC], by_k[SD]
    assert (a["launches"], a["closed"]) == (4, 4)
    assert a["mean_dur_us"] == pytest.approx(50.0) and a["mean_gap_us"] == pytest.approx(3.0) and a["period_us"] == pytest.approx(53.0)
    assert (b["launches"], b["closed"]) == (3, 3)
    assert b["mean_dur_us"] == pytest.approx(46.0) and b["mean_gap_us"] == pytest.approx(2.0 / 3.0)      # 1, -1, 2: the overlap counts
    assert b["period_us"] == pytest.approx(46.0 + 2.0 / 3.0)
    assert c["launches"] == 4 and c["mean_dur_us"] == pytest.approx(25.0) and c["mean_gap_us"] == pytest.approx(2.5)
    assert c["period_us"] == pytest.approx(27.5)
    # the last dispatch of the file: a launch with a duration, no gap and no period
    assert (d["launches"], d["closed"]) == (1, 0)
    assert d["mean_dur_us"] == pytest.approx(7.0) and d["mean_gap_us"] is None and d["period_us"] is None
    assert list(by_k)[0] == SA                                  # sorted by total period


def test_by_pair(tool, trace):
    _, by_p = tool.analyse(tool.read_trace(trace))
    assert set(by_p) == {(SA, SB), (SA, SC), (SB, SC), (SC, SA), (SC, SD)}
    want = {(SA, SB): (3, 50.0, 2.0), (SA, SC): (1, 50.0, 6.0), (SB, SC): (3, 46.0, 2.0 / 3.0), (SC, SA): (3, 25.0, 3.0),
            (SC, SD): (1, 25.0, 1.0)}
    for pair, (n, dur, gap) in want.items():
        r = by_p[pair]
        assert r["launches"] == n, pair
        assert r["mean_dur_us"] == pytest.approx(dur) and r["mean_gap_us"] == pytest.approx(gap), pair
        assert r["period_us"] == pytest.approx(dur + gap), pair
    # every dispatch but the last is in exactly one pair
    assert sum(r["launches"] for r in by_p.values()) == len(DISPATCHES) - 1


def test_queues_do_not_chain(tool):
    rows = [(("Agent 2", "1"), "k", 0, 10), (("Agent 2", "2"), "k", 5, 30), (("Agent 2", "1"), "k", 14, 20)]
    by_k, by_p = tool.analyse(rows)
    assert by_k["k"]["launches"] == 3 and by_k["k"]["closed"] == 1 and by_k["k"]["mean_gap_us"] == pytest.approx(0.004)
    assert by_p[("k", "k")]["launches"] == 1


def test_command_line(trace):
    r = subprocess.run([sys.executable, TOOL, trace, "--match", "linear_x3d", "--json"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert set(got["kernels"]) == {SA, SC}
    assert got["kernels"][SA]["period_us"] == pytest.approx(53.0)
    assert f"{SC} -> {SD}" in got["pairs"] and f"{SB} -> {SC}" not in got["pairs"]
    r = subprocess.run([sys.executable, TOOL, trace], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    last = [l for l in r.stdout.splitlines() if l.endswith("  " + SD)]
    assert len(last) == 1 and last[0].split()[:4] == ["1", "7.00", "-", "-"]
    assert f"{SB} -> {SC}" in r.stdout
