#!/usr/bin/env python3
"""Record what tests/det_math_checks.py measures: the maxima of every check of the device's elementary functions and random draws (det_sincos, det_atan2,
det_log, box_muller, philox4x32, sqrt_), one JSON row per function and dtype, for one backend.

    python tools/det_math_exhaustive.py --backend oracle            # the CPU oracle's restatement (no GPU)
    python tools/det_math_exhaustive.py --backend hip               # the HIP library; every call is held to the oracle bit for bit first

Rows are appended to --out (default profiles/det_math_exhaustive.jsonl; rows of the same backend already there are replaced).  A check whose assertion fails is
recorded as "failed" with the message, which names the figure and its bound; the exit status is then 1."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=("oracle", "hip"), required=True)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "det_math_exhaustive.jsonl"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import det_math_checks as dm
    be = dm.OracleBackend() if a.backend == "oracle" else dm.HipBackend()
    rows = []

    def run(function, dtype, check):
        row = {"backend": a.backend, "function": function, "dtype": dtype}
        print(function, dtype or "")
        try:
            row.update(check())
        except AssertionError as e:
            row["failed"] = str(e)[:400]
        rows.append(row)

    for name, check in dm.CHECKS.items():
        for dtype in dm.DTYPES:
            run(name, dm.DTYPE_NAME[dtype], lambda: check(be, dtype))
    run("philox4x32", None, lambda: dm.check_philox(be))
    if a.backend == "hip":
        run("sqrt_", "float32", lambda: dm.check_sqrt_ieee(be))
    out = Path(a.out)
    kept = [l for l in out.read_text().splitlines() if l.strip() and json.loads(l)["backend"] != a.backend] if out.exists() else []
    out.write_text("\n".join(kept + [json.dumps(r) for r in rows]) + "\n")
    print(f"{len(rows)} rows -> {out}")
    return 1 if any("failed" in r for r in rows) else 0


if __name__ == "__main__":
    sys.exit(main())
