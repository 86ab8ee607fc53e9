"""Host side of the device-resident step outputs (Engine.view_dev, Engine.reset_dev, tensor_env), without a GPU: the refusals that are raised before the library
is touched, the observation row's order against the library's field names, the loud failure of the two C calls without a context, and that only tensor_env
brings torch into the package."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "dql_multirotor_landing_amd"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from dql_multirotor_landing_amd import _lib
    return _lib.load()


class _Untouchable:
    """stands where an Engine keeps its library: any use fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the argument was refused")


def _bare_engine(n=8):
    from dql_multirotor_landing_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.lib, e.n, e._h = _Untouchable(), n, None
    return e


@pytest.mark.parametrize("kwargs,needle", [
    ({"real_dtype": 2, "obs": 4096}, "real_dtype"),
    ({"real_dtype": -1}, "real_dtype"),
    ({"real_dtype": None, "done": 4096}, "real_dtype"),
    ({"obs": 4096 + 8}, "16-byte aligned"),
    ({"obs": 4096 + 4, "real_dtype": 1}, "16-byte aligned"),
    ({"reward": -16}, "reward"),
    ({"done": 1.5}, "done"),
    ({"code": "0x1000"}, "code"),
    ({"idx_x": True}, "idx_x"),
    ({"bad_actions": 1 << 64}, "bad_actions"),
])
def test_view_dev_refuses_before_the_library_is_touched(kwargs, needle):
    with pytest.raises(ValueError, match=needle):
        _bare_engine().view_dev(**kwargs)


def test_view_dev_takes_keywords_only():
    with pytest.raises(TypeError):
        _bare_engine().view_dev(4096)


@pytest.mark.parametrize("ptr", [0, None, -4096, 1.0, False, 1 << 64])
def test_reset_dev_refuses_before_the_library_is_touched(ptr):
    with pytest.raises(ValueError, match="reset"):
        _bare_engine().reset_dev(ptr)


def test_the_observation_row_is_the_named_fields_in_the_header_s_order(lib):
    """Engine.VIEW_OBS_FIELDS against the library's field names: field f lives in quad f // 4, component f % 4, and dql_view.hpp reads exactly these"""
    from dql_multirotor_landing_amd import _lib
    from dql_multirotor_landing_amd.engine import Engine
    names = [lib.dql_field_name(i, 0).decode() for i in range(64)]
    assert len(Engine.VIEW_OBS_FIELDS) == _lib.VIEW_OBS == 8
    where = [divmod(names.index(f), 4) for f in Engine.VIEW_OBS_FIELDS]
    assert where == [(14, 1), (14, 2), (14, 3), (7, 3), (15, 0), (15, 1), (15, 2), (10, 2)]
    assert divmod(names.index("reward"), 4) == (14, 0) and divmod(names.index("cum_x"), 4) == (10, 1)
    # ... and the header says so: the row's initialiser names the same quads and components, in this order
    hpp = (PKG / "csrc" / "dql_view.hpp").read_text()
    row = re.search(r"const R row\[VIEW_OBS\] = \{(.*?)\};", hpp, re.S).group(1)
    assert [(int(q), "abcd".index(c)) for q, c in re.findall(r"view_cast<R>\(q(\d+)\.([abcd])\)", row)] == where
    # ... and include/dql.h declares the same row length and the struct the binding mirrors, pointer for pointer
    hdr = (ROOT / "include" / "dql.h").read_text()
    assert re.search(r"#define DQL_VIEW_OBS 8\b", hdr)
    body = re.search(r"typedef struct dql_view \{(.*?)\} dql_view;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\*\s*(\w+)\s*;", body) == list(_lib.VIEW_POINTERS)
    assert [n for n, _ in _lib.DqlViewC._fields_] == ["real_dtype", "reserved", *_lib.VIEW_POINTERS]
    assert C.sizeof(_lib.DqlViewC) == 8 + 8 * len(_lib.VIEW_POINTERS)


def test_view_dev_and_reset_dev_fail_loudly_without_a_context(lib):
    """no context, no fallback: both calls return DQL_EINVAL with a sentence (an Engine cannot be made without a GPU: tests/test_abi.py)"""
    from dql_multirotor_landing_amd import _lib
    v = _lib.DqlViewC(real_dtype=0, reserved=0)
    assert lib.dql_view_dev(None, C.byref(v)) == _lib.EINVAL and b"null context" in lib.dql_last_error()
    assert lib.dql_reset_dev(None, None) == _lib.EINVAL and b"null context" in lib.dql_last_error()
    with pytest.raises(ValueError, match="null context"):
        _lib.check(lib.dql_view_dev(None, None))
    n = C.c_int(0)
    if lib.dql_device_count(C.byref(n)) != 0 or n.value == 0:
        from dql_multirotor_landing_amd.config import DqlConfig
        from dql_multirotor_landing_amd.engine import Engine
        with pytest.raises(RuntimeError):
            Engine(DqlConfig(), 8).view_dev(done=4096)


def test_only_tensor_env_brings_torch_into_the_package():
    code = ("import sys; import dql_multirotor_landing_amd as p; from dql_multirotor_landing_amd import engine, ops, _lib; "
            "assert 'torch' not in sys.modules, 'torch was imported'; assert 'dql_multirotor_landing_amd.tensor_env' not in sys.modules, 'tensor_env was imported'")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    importers = [p.name for p in PKG.glob("*.py") if re.search(r"^\s*(import torch|from torch)\b", p.read_text(), re.M)]
    assert importers == ["tensor_env.py"]
