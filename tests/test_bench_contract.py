"""The committed bench line (profiles/<ROUND>/bench.json, written by
`bench.py --full` on an MI355X) keeps the driver's contract: the BASELINE metric and unit, whole-job
throughput consistent with ms_per_step, the roofline object (bound, achieved,
peak, unit, frac = achieved / peak, traffic from the PMC passes) with the
VALU-issue evidence of profiles/<ROUND>/valu_issue.json, the world kernels'
VALU-issue rooflines (profiles/<ROUND>/world_pmc_*.json), and a bounded
cpu_baseline; the traffic figures DESIGN.md quotes are the committed PMC
JSON's.  CPU-only: it reads files, it runs nothing."""
import json
import os

from conftest import REPO

ROUND = "r06"
BENCH = os.path.join(REPO, "profiles", ROUND, "bench.json")


def load(name, rnd=ROUND):
    with open(os.path.join(REPO, "profiles", rnd, name)) as f:
        return json.load(f)


def source_round(roof, name, key):
    """The round directory whose evidence file the bench line read (lines
    without a traffic_source field: the round whose file holds the value)."""
    if "traffic_source" in roof:
        return roof["traffic_source"].split("/")[1]
    for rnd in (ROUND, "r03", "r02", "r01"):
        if os.path.exists(os.path.join(REPO, "profiles", rnd, name)) and round(load(name, rnd)[key]) == roof["traffic"]:
            return rnd
    return ROUND


def test_bench_line_contract():
    b = load("bench.json")
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert b["metric"].startswith("Msamples/sec")
    assert "Msamples/sec" in base["metric"]
    assert b["unit"] == "Msamples/s" and b["higher_is_better"] is True and b["scaling"] == "weak"
    assert b["n_gpus"] == 1 and b["dtype"] == "f64" and b["vs_baseline"] is None
    c = b["config"]
    assert (c["width"], c["height"], c["spp_frame"], c["max_depth"], c["seed"]) == (1200, 675, 500, 50, 42)
    samples = c["width"] * c["height"] * c["spp_frame"]
    # value = samples / wall time of one step (ms_per_step), within rounding
    assert abs(b["value"] - samples / (b["ms_per_step"] * 1e-3) / 1e6) / b["value"] < 0.01


def test_roofline_fields_are_consistent():
    r = load("bench.json")["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["unit"] == "TFLOP/s" and r["peak"] == 78.6
    # achieved = algorithmic flops per launch / the launch's average duration
    assert abs(r["achieved"] - r["flop_per_launch"] / (r["trace_ms_per_launch"] * 1e-3) / 1e12) < 0.01 * r["achieved"]
    t = load("traffic.json", source_round(r, "traffic.json", "traffic_bytes_per_launch"))
    assert r["traffic"] == round(t["traffic_bytes_per_launch"])
    v = load("valu_issue.json")
    assert r["valu_issue"]["busy_frac"] == v["valu_busy_frac"]
    assert r["valu_issue"]["valu_per_wave_iteration"] == v["valu_per_wave_iteration"]
    assert 0.5 < v["valu_busy_frac"] <= 1.0
    h = r["hbm"]
    assert h["unit"] == "GB/s" and h["peak"] == 8000.0 and h["frac"] < 0.01


def test_rocprof_summary_agrees_with_the_event_timing():
    import csv
    r = load("bench.json")["roofline"]
    rows = list(csv.DictReader(open(os.path.join(REPO, "profiles", ROUND, "bench_kernel_stats.csv"))))
    trace = [x for x in rows if x["Name"].startswith("void rtwk::trace_kernel<double, false, 0,")]
    assert trace, "no f64 trace_kernel row in the rocprofv3 summary"
    avg_ms = float(trace[0]["AverageNs"]) / 1e6
    assert abs(avg_ms - r["trace_ms_per_launch"]) / avg_ms < 0.05


def test_cpu_baseline_is_bounded_and_stated():
    cb = load("bench.json")["cpu_baseline"]
    assert cb["unit"] == "Msamples/s" and cb["cores"] == 1 and cb["kind"] in ("port", "reference")
    assert cb["value"] > 0 and "spp" in cb["sample"]


def test_wavefront_traffic_is_the_pmc_measurement():
    wf = load("bench.json")["wavefront_variant"]["roofline"]
    t = load("wf_traffic.json", source_round(wf, "wf_traffic.json", "traffic_bytes_per_frame"))
    assert wf["traffic"] == round(t["traffic_bytes_per_frame"])
    # the queues move close to their algorithmic bytes (no wasted re-reads; below them since round 6's
    # smaller queues let the XCDs' L2 serve part of each pass's re-read: 0.77x, profiles/r06/wf_step_ab.txt)
    assert 0.7 < wf["traffic"] / wf["algorithmic_bytes_per_frame"] < 1.5
    assert abs(wf["frac"] - wf["achieved"] / wf["peak"]) < 1e-3


def test_world_rooflines_are_the_pmc_evidence():
    b = load("bench.json")
    for key, scene in (("globe_10k_variant", 7), ("cornell_variant", 6)):
        r = b[key]["roofline"]
        t = load(f"world_pmc_{scene}.json")
        kms = b[key]["kernel_ms"]
        assert r["kernel"] == "world_kernel" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
        assert 0.3 < r["frac"] <= 1.0
        v = r.get("valu_issue", r)  # the VALU-issue figures: the roofline itself, or its side field
        if r["unit"] == "G TD-busy cycles/s":
            # the per-lane walk's bound: the TD's busy cycles of the PMC launch
            # over the bench's launch time, against every TD busy every cycle
            assert r["bound"].startswith("vmem-return (TD")
            assert abs(r["achieved"] - t["vmem_counters"]["TD_TD_BUSY_sum"] / (kms * 1e-3) / 1e9) < 0.01 * r["achieved"]
            assert abs(r["peak"] - 256 * t["clock_ghz"]) < 0.1
            assert abs(r["frac"] - t["td_busy_frac"]) < 0.1  # (PMC dispatch vs bench launch time)
        else:
            assert r["unit"] == "G wave64 VALU instructions/s"
        # VALU achieved = the launch's PMC VALU instructions / the launch time measured by the bench
        assert v["unit"] == "G wave64 VALU instructions/s" and abs(v["frac"] - v["achieved"] / v["peak"]) < 1e-3
        assert abs(v["achieved"] - t["counters"]["SQ_INSTS_VALU"] / (kms * 1e-3) / 1e9) < 0.01 * v["achieved"]
        assert abs(v["peak"] - 1024 * t["clock_ghz"] / 4) < 0.1
        assert r["traffic"] == round(t["hbm_fetch_bytes"] + t["hbm_write_bytes"])
        # the PMC dispatch and the bench's launch time agree
        assert abs(t["dispatch_ms"] - kms) / kms < 0.1


def test_design_traffic_figures_are_the_committed_json():
    """DESIGN.md §0's PMC traffic table quotes exactly the committed evidence
    (rounded as printed), so a reader never meets a stale figure."""
    import re
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    keys = {"traffic.json": "traffic_bytes_per_launch", "wf_traffic.json": "traffic_bytes_per_frame"}
    rows = re.findall(r"^\| [^|`]*\(`profiles/(r\d\d)/(\w+\.json)`\) \| \w+ \| ([\d.]+) (MB|GB) \|", text, re.M)
    assert len(rows) >= 4, rows
    for rnd, name, val, unit in rows:
        assert rnd == ROUND, (rnd, name)
        t = load(name, rnd)
        b = t[keys[name]] if name in keys else t["hbm_fetch_bytes"] + t["hbm_write_bytes"]
        scale = 1e6 if unit == "MB" else 1e9
        digits = len(val.split(".")[1]) if "." in val else 0
        assert abs(float(val) - b / scale) <= 0.5 * 10 ** -digits + 1e-12, (name, val, unit, b)


def test_design_has_no_unfilled_template_tokens():
    """DESIGN.md once carried unfilled placeholders
    (`PORT_BOX`, `TIERA_BOX`).  Upper-case snake tokens of that shape that are
    not identifiers of this repository (RTW_* macros and env names, rtw_hip.h
    constants, file names) must not appear."""
    import re
    txt = open(os.path.join(REPO, "DESIGN.md")).read()
    known = set(re.findall(r"\b[A-Z][A-Z0-9]*(?:_[A-Z0-9]+)+\b", open(os.path.join(REPO, "include", "rtw_hip.h")).read()))
    bad = []
    for tok in set(re.findall(r"\b[A-Z][A-Z0-9]*(?:_[A-Z0-9]+)+\b", txt)):
        if tok.startswith(("RTW_", "RO_", "DRTW_", "DBL_", "FLT_", "SQ_", "TCC_", "TCP_", "TD_", "TA_", "GRBM_", "HSA_", "GPU_",
                           "HIP_", "OMP_", "MAX_")) or tok in known:  # (RO_: oracle/rtw_oracle.h macros)
            continue
        if tok in ("FETCH_SIZE", "WRITE_SIZE", "VAR_BIT", "TIER_A", "TIER_B") or tok.endswith(("_MHZ", "_MS")):
            continue
        bad.append(tok)
    assert not bad, sorted(bad)


def test_wavefront_rooflines_count_the_bounces_per_launch():
    """with --engine wavefront --wf-bounces K the headline roofline
    counted the queue bytes of K = 1 (K times too many).  Both wavefront
    rooflines take their bytes from bench.wf_frame_bytes: the fused form
    crosses the queues once per K segments, the split form once per segment."""
    import importlib
    import sys
    from types import SimpleNamespace
    sys.path.insert(0, REPO)
    bench = importlib.import_module("bench")
    counts = {"segments": 1_000_000, "samples": 400_000, "drain_segments": 50_000}
    units = 30_000
    for k in (0, 1, 3):
        a = SimpleNamespace(wf_form="fused", wf_bounces=k, precision="f64")
        assert bench.wf_frame_bytes(a, counts, units) == bench.wavefront_bytes(counts, "f64", units, True, max(k, 1))
    a3 = SimpleNamespace(wf_form="fused", wf_bounces=3, precision="f64")
    a1 = SimpleNamespace(wf_form="fused", wf_bounces=1, precision="f64")
    fixed = counts["samples"] * (2 * (24 + 4) + 4) + units * 24
    q1, q3 = bench.wf_frame_bytes(a1, counts, units) - fixed, bench.wf_frame_bytes(a3, counts, units) - fixed
    assert q1 == 950_000 * 200 and q3 == 950_000 * 200 // 3  # 200 B per queued f64 segment
    sp = SimpleNamespace(wf_form="split", wf_bounces=3, precision="f64")
    assert bench.wf_frame_bytes(sp, counts, units) == bench.wavefront_bytes(counts, "f64", units, False, 1)
    # the headline path and the variant line both call it
    src = open(os.path.join(REPO, "bench.py")).read()
    assert src.count("= wf_frame_bytes(args, ") == 2 and "wavefront_bytes(rend.counts" not in src


def test_design_pmc_shares_are_the_committed_json():
    """the pipe shares and write bytes DESIGN.md §0 quotes for the
    world kernel (VALU busy, TD busy, TA busy, WRITE_SIZE per launch) are the
    committed PMC JSON's, rounded as printed."""
    import re
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    rows = re.findall(r"^\| [^|`]*\(`profiles/(r\d\d)/(world_pmc_\d\.json)`\) \| ([\d.]+) \| ([\d.]+) \| ([\d.]+) \| "
                      r"([\d.]+) GB \|", text, re.M)
    assert len(rows) == 2, rows
    for rnd, name, valu, td, ta, wr in rows:
        assert rnd == ROUND, (rnd, name)
        t = load(name, rnd)
        for quoted, val in ((valu, t["valu_busy_frac"]), (td, t["td_busy_frac"]), (ta, t["ta_busy_frac"]),
                            (wr, t["hbm_write_bytes"] / 1e9)):
            digits = len(quoted.split(".")[1])
            assert abs(float(quoted) - val) <= 0.5 * 10 ** -digits + 1e-12, (name, quoted, val)
    # the globe's write-back of round 5's in-loop spill is gone (VERDICT r5 ask 1: <= 0.2 GB per launch)
    assert load("world_pmc_7.json")["hbm_write_bytes"] <= 0.2e9
