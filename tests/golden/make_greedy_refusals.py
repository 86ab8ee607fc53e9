#!/usr/bin/env python3
"""greedy_refusals.json: what each of the 11 entry points of the greedy-flight family answers to every refused call of tests/greedy_refusal_checks.py, as
(return code, dql_last_error text).  Needs an MI355X (a valid call seeds each operator's last-call record, the twins need an ensemble); the library is the one
dql_multirotor_landing_amd._lib loads (DQL_LIB_PATH selects another build).  The fixture is recorded once, from the library as it stood BEFORE a change to the
family's host code, and committed as is: tests/test_gpu_greedy_refusals.py holds every later build to it, to the letter.

    python tests/golden/make_greedy_refusals.py             # print the rows, write nothing
    python tests/golden/make_greedy_refusals.py --record    # write tests/golden/greedy_refusals.json (or the path given after --record)
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent.parent), str(HERE.parent)]

import greedy_refusal_checks as grc  # noqa: E402


def main(argv):
    table = {entry: grc.rows_of(entry) for entry in grc.ENTRY_POINTS}
    n_rows = sum(len(r) for r in table.values())
    if "--record" in argv:
        i = argv.index("--record")
        out = Path(argv[i + 1]) if len(argv) > i + 1 else HERE / "greedy_refusals.json"
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(table, indent=1, sort_keys=True) + "\n")
        print(f"{n_rows} rows of {len(table)} entry points -> {out}")
    else:
        print(json.dumps(table, indent=1, sort_keys=True))
        print(f"{n_rows} rows of {len(table)} entry points (not written: pass --record)")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
