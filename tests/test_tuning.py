"""The tuning-knob table (ringsnark_amd/csrc/tuning.hpp) through rs_set_tuning / rs_get_tuning / rs_tuning_key, and the scoped
override ringsnark_amd._lib.tuning.  No device is touched: the knobs are host variables of the library.

tests/golden/tuning_table.json (tests/golden/make_tuning_golden.py) is what the release library answered before the table
existed: the status of every (key, probe value), each key's default and the value an accepted set stores; the
experiments-only key is unknown to it.  Every test leaves every knob at its default (one process with the other tests)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

from ringsnark_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "tuning_table.json")))
DEFAULTS = {k: e["default"] for k, e in FIXTURE["keys"].items() if not e["experiments"]}


def _current():
    return {k: _lib.get_tuning(k) for k in _lib.tuning_keys()}


def test_set_and_get_reproduce_the_recorded_behaviour():
    lib = _lib.load()
    for key, e in FIXTURE["keys"].items():
        if e["experiments"]:
            continue
        with _lib.tuning(**{key: e["default"]}):  # the default is itself an accepted value
            for value, status, stored in zip(FIXTURE["values"], e["status"], e["stored"]):
                before = _lib.get_tuning(key)
                assert lib.rs_set_tuning(key.encode(), value) == status, (key, value)
                assert _lib.get_tuning(key) == (stored if status == _lib.RS_OK else before), (key, value)
        assert _lib.get_tuning(key) == e["default"], key
    unknown = [k for k, e in FIXTURE["keys"].items() if e["experiments"]] + [FIXTURE["unknown_key"]["name"]]
    for key in unknown:
        statuses = FIXTURE["keys"][key]["status"] if key in FIXTURE["keys"] else FIXTURE["unknown_key"]["status"]
        for value, status in zip(FIXTURE["values"], statuses):
            assert lib.rs_set_tuning(key.encode(), value) == status == _lib.RS_ERR_INVALID, (key, value)
        out = C.c_int(-77)
        assert lib.rs_get_tuning(key.encode(), C.byref(out)) == _lib.RS_ERR_INVALID and out.value == -77, key
    assert _current() == DEFAULTS


def test_rejections_keep_their_messages():
    lib = _lib.load()
    for key, value, code, text in [("witness_lds_logM", 14, _lib.RS_ERR_INVALID, "witness_lds_logM must be in [6, 13]"),
                                   ("witness_sub_log", 14, _lib.RS_ERR_INVALID, "witness_sub_log must be 12 or 13"),
                                   ("msm_c_mib", 0, _lib.RS_ERR_INVALID, "msm_c_mib must be positive"),
                                   ("witness_big_ws_mib", 63, _lib.RS_ERR_INVALID, "witness_big_ws_mib must be at least 64"),
                                   ("witness_force_bc", 4, _lib.RS_ERR_INVALID, "witness_force_bc must be 0 or in [5, 20]"),
                                   ("witness_sub_ct", 1, _lib.RS_ERR_UNSUPPORTED, "witness_sub_ct 1 and 3 exist in the experiments build only"),
                                   ("no_such_knob", 0, _lib.RS_ERR_INVALID, "unknown tuning key no_such_knob")]:
        assert lib.rs_set_tuning(key.encode(), value) == code, key
        assert lib.rs_last_error().decode() == text
    assert lib.rs_get_tuning(b"ntt_variant", None) == _lib.RS_ERR_INVALID and lib.rs_set_tuning(None, 0) == _lib.RS_ERR_INVALID


def test_key_enumeration_is_the_table():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ringsnark_amd", "tuning.h")).read()
    assert set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", hdr)) == set(_lib.TUNING_SIGNATURES)  # as tests/test_cabi.py does
    keys = _lib.tuning_keys()
    assert sorted(keys) == sorted(DEFAULTS) and len(set(keys)) == len(keys)
    assert lib.rs_tuning_key(-1) is None and lib.rs_tuning_key(len(keys)) is None and lib.rs_tuning_key(1 << 30) is None


def test_a_fresh_process_reports_every_default():
    code = ("import json, sys; sys.path.insert(0, %r); from ringsnark_amd import _lib; "
            "print(json.dumps({k: _lib.get_tuning(k) for k in _lib.tuning_keys()}))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, cwd=ROOT).stdout
    assert json.loads(out.strip().splitlines()[-1]) == DEFAULTS


def test_scoped_override_restores():
    # normal exit; stored values are the normalised ones
    with _lib.tuning(witness_lds_logM=6, mac_chunk_units=-5, witness_h_coset=7):
        assert (_lib.get_tuning("witness_lds_logM"), _lib.get_tuning("mac_chunk_units"), _lib.get_tuning("witness_h_coset")) == (6, 1, 1)
        with _lib.tuning(witness_lds_logM=8):  # nested: back to the enclosing value, not to the default
            assert _lib.get_tuning("witness_lds_logM") == 8
        assert _lib.get_tuning("witness_lds_logM") == 6
    assert _current() == DEFAULTS
    # an exception in the body
    with pytest.raises(ZeroDivisionError):
        with _lib.tuning(witness_force_bc=14, witness_inc=0):
            assert _lib.get_tuning("witness_force_bc") == 14
            raise ZeroDivisionError
    assert _current() == DEFAULTS
    # a failing set in the middle of the argument list: the knobs before it are restored, the ones after it never set
    with pytest.raises(_lib.RsError) as err:
        with _lib.tuning(witness_lds_logM=6, witness_sub_ct=1, mac_variant=3):
            pytest.fail("the body must not run")
    assert err.value.code == _lib.RS_ERR_UNSUPPORTED
    assert _current() == DEFAULTS


def test_tuning_from_env(monkeypatch):
    monkeypatch.setenv("RS_TUNING", "witness_sub_ct=0,ntt_variant=12")
    with _lib.tuning(witness_sub_ct=DEFAULTS["witness_sub_ct"], ntt_variant=DEFAULTS["ntt_variant"]):
        _lib.tuning_from_env("RS_TUNING_OF_NOBODY")  # unset: nothing changes
        assert _current() == DEFAULTS
        _lib.tuning_from_env()
        assert (_lib.get_tuning("witness_sub_ct"), _lib.get_tuning("ntt_variant")) == (0, 12)
    assert _current() == DEFAULTS
