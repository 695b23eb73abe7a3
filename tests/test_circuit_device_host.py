"""The device-resident circuit runs (sgfhe_circuit_run*_device, include/sgfhe_hip.h) as far as a machine without a GPU
sees them: the four entries are declared and exported with the arity of their host entry plus the stream, the ABI
revision is unchanged, a NULL ctx is refused before anything else, and the tensor validator of the Python forms
(check_device_tensor) names each defect of an argument before any library call.  The runs themselves:
tests/test_gpu_circuit_device.py."""

import os
import re

import pytest

INVALID = -1                               # SGFHE_ERR_INVALID_ARG
ARITY = {"sgfhe_circuit_run_device": 7, "sgfhe_circuit_run_ct_device": 12,
         "sgfhe_circuit_run_steps_device": 11, "sgfhe_circuit_run_steps_ct_device": 17}
HOST_FORM = {"sgfhe_circuit_run_device": "sgfhe_circuit_run_data", "sgfhe_circuit_run_ct_device": "sgfhe_circuit_run_ct_data",
             "sgfhe_circuit_run_steps_device": "sgfhe_circuit_run_steps",
             "sgfhe_circuit_run_steps_ct_device": "sgfhe_circuit_run_steps_ct"}


def _declarations():
    """name -> the parameter list of its declaration in include/sgfhe_hip.h, comments removed."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "sgfhe_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint32_t\s+(sgfhe_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}


def test_entries_declared_and_exported(S):
    decl = _declarations()
    for name, arity in ARITY.items():
        assert name in decl, name
        assert name in S.EXPORTED_SYMBOLS, name
        assert len(decl[name]) == arity, (name, decl[name])
        assert re.fullmatch(r"void\s*\*\s*stream", decl[name][-1]), decl[name][-1]
        # the most general host entry of the form, plus the stream
        assert [re.sub(r"\s+", " ", a) for a in decl[name][:-1]] == [re.sub(r"\s+", " ", a) for a in decl[HOST_FORM[name]]]
        fn = getattr(S.lib(), name)
        assert len(fn.argtypes) == arity


def test_abi_revision_unchanged(S):
    assert S.lib().sgfhe_abi_version() == 7 and S.ABI_VERSION == 7


def test_null_ctx_is_refused(S):
    L = S.lib()
    for name, arity in ARITY.items():
        args = [None if t is not None and getattr(t, "_type_", None) == "P" else 0 for t in getattr(L, name).argtypes]
        assert len(args) == arity
        assert getattr(L, name)(*args) == INVALID, name


def test_tensor_validator(S):
    """Each of the six defects, by its own message; CPU and meta tensors only: no GPU, no engine, no library call."""
    import numpy as np
    import torch
    check = S.check_device_tensor
    shape = (3, 8, 65)
    good = torch.zeros(shape, dtype=torch.int64, device="meta")
    with pytest.raises(ValueError, match="torch.Tensor is needed"):
        check("inputs", np.zeros(shape, dtype=np.uint64), shape, 0)
    with pytest.raises(ValueError, match="CPU tensor"):
        check("inputs", torch.zeros(shape, dtype=torch.int64), shape, 0)
    with pytest.raises(ValueError, match="is on meta"):                      # a device that is not the engine's
        check("inputs", good, shape, 0)
    for bad in (torch.int32, torch.float64, torch.uint8):
        with pytest.raises(ValueError, match="dtype must be torch.int64 or torch.uint64"):
            check("inputs", torch.zeros(shape, dtype=bad), shape, 0)
    with pytest.raises(ValueError, match="dtype must be torch.uint8"):
        check("data", torch.zeros((2, 8), dtype=torch.int64), (2, 8), 0, words=False)
    with pytest.raises(ValueError, match="must be contiguous"):
        check("inputs", torch.zeros((3, 65, 8), dtype=torch.int64).transpose(1, 2), shape, 0)
    with pytest.raises(ValueError, match="must be contiguous"):
        check("inputs", torch.zeros((3, 16, 65), dtype=torch.int64)[:, ::2], shape, 0)
    for wrong in ((3, 8, 64), (2, 8, 65), (3, 8), (1, 3, 8, 65)):
        with pytest.raises(ValueError, match="shape must be"):
            check("inputs", torch.zeros(wrong, dtype=torch.int64), shape, 0)
    with pytest.raises(ValueError, match="shape must be"):                   # None matches any length, not any rank
        check("inputs", torch.zeros((3, 8), dtype=torch.uint64), (3, None, 65), 0)
    # a well-formed CPU tensor gets as far as the device check, with either word dtype and a free axis
    for dt in (torch.int64, torch.uint64):
        with pytest.raises(ValueError, match="CPU tensor"):
            check("inputs", torch.zeros((3, 24, 65), dtype=dt), (3, None, 65), 0)
    with pytest.raises(ValueError, match="CPU tensor"):
        check("data", torch.zeros((2, 8), dtype=torch.uint8), (2, 8), 0, words=False)


def test_methods_validate_before_the_library(S):
    """The Engine methods raise on a CPU tensor without a ctx: the check comes before any library call."""
    import torch
    eng = S.Engine.__new__(S.Engine)                 # no ctx: any library call would fail on the missing handle
    eng.params, eng.device, eng._h = S.Params(64), 0, None
    c = S.Circuit(2)
    c.output(c.gate(*c.inputs)[0])
    x = torch.zeros((2, 8, 65), dtype=torch.int64)
    with pytest.raises(ValueError, match="CPU tensor"):
        eng.circuit_run_device(c, x)
    with pytest.raises(ValueError, match="CPU tensor"):
        eng.circuit_run_ct_device(c, torch.zeros((2, 1, 64), dtype=torch.int64), torch.zeros((2, 1, 64), dtype=torch.int64))
    with pytest.raises(ValueError, match="CPU tensor"):
        eng.circuit_run_steps_device(c, None, torch.zeros((3, 2, 8, 65), dtype=torch.int64))
    with pytest.raises(ValueError, match="CPU tensor"):
        eng.circuit_run_steps_ct_device(c, None, None, torch.zeros((3, 2, 1, 64), dtype=torch.int64),
                                        torch.zeros((3, 2, 1, 64), dtype=torch.int64))
