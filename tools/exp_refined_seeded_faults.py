"""Seeded faults of the refined-state bodies: each fault is applied to a scratch copy of csrc/dql_refined.hpp (one of them to a scratch
copy of the emulation driver, whose transfer loop restates dql_ensemble_transfer over 2 n table sets), tests/host_emu/refined_emu.cpp is built against the copy,
plain and sanitized, and tests/test_refined_host_emulation.py is run through it, one child process per fault.  Prints, per fault, how many of the module's rows
turned red and which, grouped by the module's cases (a) .. (e).  CPU only; about a minute per fault, the faults in parallel.

    python tools/exp_refined_seeded_faults.py [--keep DIR] [--only NAME[,NAME...]] [--jobs 5]
"""
import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER, DRIVER = ROOT / "dql_multirotor_landing_amd" / "csrc" / "dql_refined.hpp", ROOT / "tests" / "host_emu" / "refined_emu.cpp"
LOAD_NEXT = "const QRow next = load_qrow((const double*)qa, (const double*)qb, rx);"
SCORE_HALF = "      const int sx = refined_state(e.idx_x);\n      hb = refined_half(feature, e, j + 1, env_id, (uint32_t)seed, cut[sx]);"
# name -> ("header" | "driver", [(text, replacement)]): every text must occur exactly once in the file
FAULTS = {
    "none": ("header", []),
    "the half taken with j instead of j + 1": ("header", [("(int)(uint32_t)(j0 + p + 1)", "(int)(uint32_t)(j0 + p)"), ("refined_half(feature, e, j + 1,", "refined_half(feature, e, j,")]),
    "> for >=": ("header", [("value >= at ? 1 : 0", "value > at ? 1 : 0")]),
    "the cut indexed by the state before the period": ("header", [
        ("const int prev_p = e.bin_p, hb_before = hb;", "const int prev_p = e.bin_p, hb_before = hb, sx_before = refined_state(e.idx_x);"),
        ("(uint32_t)seed, rf.cut[sx]);", "(uint32_t)seed, rf.cut[sx_before]);"), (SCORE_HALF, SCORE_HALF.replace("cut[sx]", "cut[refined_state(before_x)]"))]),
    "the bootstrap row taken from the half of s": ("header", [
        (LOAD_NEXT, "const QRow next = load_qrow((const double*)qa, (const double*)qb, (hb_before & 1) * DQL_N_STATES + sx);"),
        ("      qx = next;\n", "      qx = load_qrow((const double*)qa, (const double*)qb, rx);\n")]),
    "the patch done by unrefined index": ("header", [("qrow_patch(qx, rx, cell, sel_b, q_new);", "qrow_patch(qx, sx, sa, sel_b, q_new);")]),
    "the half recomputed from the loaded env at a launch boundary": ("header", [
        ("hb = rf.half[l] & 3;", "hb = refined_half(rf.feature, e, (int)(uint32_t)j0, (uint32_t)l, (uint32_t)seed, rf.cut[refined_state(e.idx_x)]);")]),
    "the count kept per unrefined cell": ("header", [("const double cnt = count[cell];", "const double cnt = count[sa];"), ("count[cell] = cnt + 1.0;", "count[sa] = cnt + 1.0;")]),
    "transfer of half 0 only": ("driver", [("for (long long set = 0; set < 2 * h.n; ++set) {", "for (long long set = 0; set < 2 * h.n; set += 2) {")]),
    "scoring that always reads half 0": ("header", [("qx = load_qrow(qa, qb, (hb & 1) * DQL_N_STATES + sx);", "qx = load_qrow(qa, qb, sx);")]),
}


def child(name, work):
    """apply the fault to scratch copies under `work`, point the harness at them, run the emulation module, print the red rows"""
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
    which, edits = FAULTS[name]
    text = {"header": HEADER.read_text(), "driver": DRIVER.read_text()}
    for old, new in edits:
        assert text[which].count(old) == 1, f"{name}: {old!r} occurs {text[which].count(old)} times"
        text[which] = text[which].replace(old, new)
    work = Path(work)
    shutil.rmtree(work, ignore_errors=True)
    (work / "inc").mkdir(parents=True)
    shutil.copytree(ROOT / "tests" / "host_emu", work / "host_emu")
    (work / "inc" / "dql_refined.hpp").write_text(text["header"])
    (work / "host_emu" / "refined_emu.cpp").write_text(text["driver"])
    import host_emu_harness as heh
    import pytest
    heh.EMU = work / "host_emu"                                   # the driver (and its neighbours) from the copy ...
    heh.PLAIN_FLAGS = ["-I", str(work / "inc")] + heh.PLAIN_FLAGS  # ... and the faulted header in front of csrc/
    heh.SAN_FLAGS = ["-I", str(work / "inc")] + heh.SAN_FLAGS

    class Rows:
        red, green = [], 0

        def pytest_runtest_logreport(self, report):
            if report.when == "call" and report.failed:
                Rows.red.append(report.nodeid.split("::")[1])
            elif report.when == "call":
                Rows.green += 1

    pytest.main([str(ROOT / "tests" / "test_refined_host_emulation.py"), "-q", "-p", "no:cacheprovider", "--tb=no", "--basetemp", str(work / "tmp")], plugins=[Rows()])
    groups = {}
    for r in Rows.red:
        m = re.match(r"test_([a-e])_", r)
        groups[m.group(1) if m else "?"] = groups.get(m.group(1) if m else "?", 0) + 1
    print(f"FAULT {name!r}: {len(Rows.red)} red of {len(Rows.red) + Rows.green} rows, by case {dict(sorted(groups.items()))}")
    for r in Rows.red:
        print("  RED", r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keep", default=None, help="directory for the scratch copies and builds (default: a temporary one)")
    ap.add_argument("--only", default=None, help="comma-separated fault names (default: all, the unfaulted copy first)")
    ap.add_argument("--jobs", type=int, default=5)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--work", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.work)
    names = list(FAULTS) if not a.only else [n for n in a.only.split(",")]
    bad = [n for n in names if n not in FAULTS]
    if bad:
        ap.error(f"no fault named {bad}: one of {list(FAULTS)}")
    with tempfile.TemporaryDirectory() as tmp:
        base = Path(a.keep or tmp)

        def fly(k):
            r = subprocess.run([sys.executable, __file__, "--child", names[k], "--work", str(base / f"fault_{k}")], capture_output=True, text=True)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("FAULT", "  RED"))]
            return "\n".join(lines) if lines else f"FAULT {names[k]!r}: the run did not finish\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}"

        with ThreadPoolExecutor(max(1, a.jobs)) as ex:
            out = list(ex.map(fly, range(len(names))))
    print("\n".join(out))
    quiet = [n for n, o in zip(names, out) if n != "none" and " 0 red of" in o.splitlines()[0]]
    if quiet:
        print("faults that turned no row red:", quiet)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
