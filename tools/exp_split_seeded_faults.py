"""Seeded faults of the split transition model's per-lane body: each fault is applied to a scratch copy of csrc/dql_model_split.hpp, the
host emulation tests/host_emu/split_model_emu.cpp is built against the copy, and every case x feature of tests/split_model_checks.py (plus the crafted
equal-to-cut arrays) is flown through it and compared with the yardstick.  Prints, per fault, which comparisons turned red.  CPU only.

    python tools/exp_split_seeded_faults.py [--keep DIR]
"""
import argparse
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))

RINT = "(long long)__builtin_rint(value * (double)(1 << DQL_SPLIT_FRAC_BITS))"
BEFORE = "DQL_DEV void before(int j, const E& e) { value = split_feature(feature, e, j, env_id, seed32); }"
FEATURE_LINE = f"      sink.feature(before_x, {RINT});\n"
# name -> [(text, replacement)]: every text must occur exactly once in the header
FAULTS = {
    "the value read after the period": [(BEFORE, "DQL_DEV void before(int j, const E&) { value = (double)j; }"),
                                        ("    const int action = e.action & 3, next", "    value = split_feature(feature, e, (int)value, env_id, seed32);\n    const int action = e.action & 3, next")],
    "> for >=": [("value >= at ? 1 : 0", "value > at ? 1 : 0")],
    "the halves swapped": [("value >= at ? 1 : 0", "value >= at ? 0 : 1")],
    "the feature sum also taken in reset periods": [(BEFORE, BEFORE[:-2] + f" if ((unsigned)e.idx_x < (unsigned)DQL_N_STATES) sink.feature(e.idx_x, {RINT}); }}"), (FEATURE_LINE, "")],
    "the coin with j + 1": [("(uint32_t)j * 0x85EBCA77u", "(uint32_t)(j + 1) * 0x85EBCA77u")],
    "the cut indexed by s'": [("cut[state_ok ? before_x : 0]", "cut[(unsigned)next < (unsigned)DQL_N_STATES ? next : 0]")],
    "PREV_ACTION without its mask": [("(double)(e.action & 3)", "(double)e.action")],
    "truncation for rint": [(FEATURE_LINE, FEATURE_LINE.replace(RINT, "(long long)(value * (double)(1 << DQL_SPLIT_FRAC_BITS))"))],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="directory for the scratch copies and builds (default: a temporary one)")
    a = ap.parse_args()
    import host_emu_harness as heh
    import split_model_checks as sc
    import test_split_model_host_emulation as t
    src = (heh.CSRC / "dql_model_split.hpp").read_text()
    work = Path(a.keep or tempfile.mkdtemp(prefix="split_faults_"))
    flights = {c: sc.flight(c) for c in sc.CASE_IDS}
    jobs = [(c, f, None) for c in sc.CASE_IDS for f in range(len(sc.FEATURES))] + [(c, sc.EQUAL_TO_CUT_FEATURE, "crafted") for c in ("A", "B64")]
    for name, edits in FAULTS.items():
        d = work / "".join(ch if ch.isalnum() else "_" for ch in name)
        d.mkdir(parents=True, exist_ok=True)
        text = src
        for old, new in edits:
            assert text.count(old) == 1, (name, old)
            text = text.replace(old, new)
        (d / "dql_model_split.hpp").write_text(text)
        exe = d / "split_model_emu_plain"
        r = subprocess.run([heh.clangxx(), *heh.PLAIN_FLAGS, "-I", str(d), "-I", str(heh.EMU), "-I", str(heh.CSRC), "-Wno-pass-failed", str(heh.EMU / "split_model_emu.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]

        def red(job):
            case_id, f, crafted = job
            cut = sc.equal_to_cut(flights[case_id]) if crafted else sc.cut_of(flights[case_id], f)
            tmp = d / f"{case_id}_{f}_{crafted}"
            tmp.mkdir(exist_ok=True)
            try:
                got = t.fly(exe, case_id, f, cut, tmp)
                sc.assert_split_set_equal(got, 0, sc.expected(flights[case_id], f, cut), "")
                return None
            except AssertionError as e:
                return f"{case_id}/{sc.FEATURES[f]}{'/crafted cut' if crafted else ''}: {str(e).strip().splitlines()[0][:90]}"

        with ThreadPoolExecutor(16) as ex:
            reds = [x for x in ex.map(red, jobs) if x]
        print(f"## {name}: {len(reds)} of {len(jobs)} comparisons red")
        for x in reds[:6]:
            print("   ", x)
        if len(reds) > 6:
            print("    ... and", len(reds) - 6, "more:", sorted({x.split(':')[0] for x in reds[6:]})[:40])


if __name__ == "__main__":
    main()
