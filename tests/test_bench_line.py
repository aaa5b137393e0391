"""bench.py's stdout result line on CPU: a full round-6 record (profiles/r6_final_bench_driver_args.json, 21 KB) goes through
result_line() and comes out as strict JSON under LINE_LIMIT bytes, with the headline fields exactly as measured."""
import importlib.util
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_result_line_of_a_full_record_is_small_strict_json():
    b = _bench()
    full = json.loads(open(os.path.join(ROOT, "profiles", "r6_final_bench_driver_args.json")).read().strip().splitlines()[-1])
    full["cpu_baseline"]["nan_entry"] = float("nan")
    text = json.dumps(b.result_line(full), allow_nan=False)
    assert len(text) <= b.LINE_LIMIT
    line = json.loads(text)
    for k in b.HEADLINE:
        assert line[k] == full[k], k
    assert line["ms_per_step"] > 0 and line["cpu_baseline"]["nan_entry"] is None
    assert line["roofline"]["frac"] == float("%.6g" % full["roofline"]["frac"])


def test_result_line_falls_back_to_the_headline_when_too_long():
    b = _bench()
    rec = {"metric": "m", "value": 1.5, "unit": "frames/s", "steps": 3, "ms_per_step": 2.0,
           "big": {"k%d" % i: math.pi * i for i in range(2000)}}
    line = b.result_line(rec)
    assert line == {"metric": "m", "value": 1.5, "unit": "frames/s", "steps": 3, "ms_per_step": 2.0}


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr
