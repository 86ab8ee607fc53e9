"""TensorEnv on the GPU (run with -m gpu on an MI355X): one test, which runs tests/tensor_env_checks.py as a child process — torch has to be imported before
the library is loaded, and this process may have loaded the library long ago.  The child closes the policy loop on the device and holds it to dql_score's
episodes, then holds every tensor of TensorEnv.step to a twin engine fed through the host (see its docstring).  A child that ends by a signal or at the time
limit fails the test, and nothing further is started."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LIMIT_S = 300


def test_tensor_env_closes_the_loop_on_the_device_and_equals_its_twin():
    pytest.importorskip("torch")
    try:
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "tensor_env_checks.py")], cwd=ROOT, capture_output=True, text=True, timeout=LIMIT_S, env=dict(os.environ))
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the child did not end within {LIMIT_S} s (hung?); its last output:\n{(e.stdout or b'')[-2000:]!r}\n{(e.stderr or b'')[-2000:]!r}")
    assert r.returncode >= 0, f"the child was ended by signal {-r.returncode}:\n{r.stderr[-4000:]}"
    assert r.returncode == 0, f"the child failed:\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    line = [l for l in r.stdout.splitlines() if l.startswith("TENSOR_ENV_REPORT ")]
    assert len(line) == 1, r.stdout[-2000:]
    report = json.loads(line[0].split(" ", 1)[1])
    print(line[0])  # which ordering mechanism ran is part of the report (pytest -s, or the failure output)
    loops = report["closed_loop"]
    assert [l["asked"] for l in loops] == ["stream", "sync"] and loops[1]["ran"] == "sync" and loops[0]["ran"] in ("stream", "sync")
    assert loops[0]["by_code"] == loops[1]["by_code"] and loops[0]["steps_sum"] == loops[1]["steps_sum"] > 0
    assert all(d > 0 for d in report["twin_done"])
