#!/usr/bin/env python3
"""ensemble_host.json: what the host code of the sequential learners answers to every refused call of tests/ensemble_host_checks.py, as (return code,
dql_last_error text), and what dql_ensemble_run shows after every call of the scripts there (launches, period index, live and unfinished learners, a hash of
the learners).  Needs an MI355X; the library is the one dql_multirotor_landing_amd._lib loads (DQL_LIB_PATH selects another build).  The fixture is recorded
once, from the library as it stood BEFORE a change to the learners' host code, and committed as is: tests/test_gpu_ensemble_host.py holds every later build
to it, to the letter.

    python tests/golden/make_ensemble_host.py             # print the tables, write nothing
    python tests/golden/make_ensemble_host.py --record    # write tests/golden/ensemble_host.json (or the path given after --record)
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent.parent), str(HERE.parent)]

import ensemble_host_checks as ehc  # noqa: E402


def main(argv):
    states = {}
    try:
        refusals = {entry: ehc.rows_of(entry, states) for entry in ehc.ENTRY_POINTS}
    finally:
        ehc.close_all(states)
    runs = {}
    for (mode, dtype), name in zip(ehc.SCRIPTS, ehc.SCRIPT_IDS):
        runs[name] = ehc.script_of(mode, dtype)
        ehc.assert_script_is_what_it_is_for(mode, runs[name])
    table = {"refusals": refusals, "runs": runs}
    n_rows, n_calls = sum(len(r) for r in refusals.values()), sum(len(p) for s in runs.values() for p in s.values())
    if "--record" in argv:
        i = argv.index("--record")
        out = Path(argv[i + 1]) if len(argv) > i + 1 else HERE / "ensemble_host.json"
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
        print(f"{n_rows} refusals of {len(refusals)} entry points, {n_calls} run calls of {len(runs)} scripts -> {out}")
    else:
        print(json.dumps(table, indent=1, sort_keys=True))
        print(f"{n_rows} refusals of {len(refusals)} entry points, {n_calls} run calls of {len(runs)} scripts (not written: pass --record)")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
