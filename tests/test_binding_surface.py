"""CPU checks of the Python binding's surface: every public name, signature, record layout and struct of ribbit_amd as
tests/golden/binding_surface.json recorded them (additions are allowed, so a new feature only appends), a signature for every
symbol of the header, and the messages the shared helpers raise."""
import ctypes as C
import inspect
import json
import os
import types

import numpy as np
import pytest

import ribbit_amd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_surface.json")


def surface() -> dict:
    """what the golden file holds, read off the imported package"""
    public = {n: v for n, v in vars(ribbit_amd).items() if not n.startswith("_") and not isinstance(v, types.ModuleType)}

    def kind(v):
        if inspect.isclass(v):
            return "structure" if issubclass(v, C.Structure) else "exception" if issubclass(v, BaseException) else "class"
        return "function" if inspect.isfunction(v) else "dtype" if isinstance(v, np.dtype) else type(v).__name__

    def ctype(t):          # (an array type's module is that of whoever made it first in this process: leave it out)
        return f"{ctype(t._type_)} * {t._length_}" if issubclass(t, C.Array) else t.__name__

    out = {"names": {n: kind(v) for n, v in public.items()}, "signatures": {}, "dtypes": {}, "structures": {}}
    for n, v in public.items():
        if inspect.isfunction(v):
            out["signatures"][n] = str(inspect.signature(v))
        elif inspect.isclass(v) and issubclass(v, C.Structure):
            out["structures"][n] = [[f, ctype(t)] for f, t in v._fields_]
        elif inspect.isclass(v) and not issubclass(v, BaseException):
            for m, f in vars(v).items():
                if inspect.isfunction(f) and (m == "__init__" or not m.startswith("_")):
                    out["signatures"][f"{n}.{m}"] = str(inspect.signature(f))
        elif isinstance(v, np.dtype):
            out["dtypes"][n] = [list(f) for f in v.descr]
    return out


def test_surface_is_unchanged():
    want, got = json.load(open(GOLDEN)), json.loads(json.dumps(surface()))
    assert any(n.startswith("Scanner.record_") for n in want["signatures"]) and want["dtypes"] and want["structures"]
    for section, entries in want.items():
        for name, value in entries.items():
            assert name in got[section], f"{section}: {name} is gone"
            assert got[section][name] == value, f"{section}: {name} changed"
    for name, k in want["names"].items():          # the file itself is whole: a signature per function, fields per struct
        assert name in want[{"function": "signatures", "structure": "structures", "dtype": "dtypes"}.get(k, "names")]


def test_every_abi_symbol_has_a_signature(hip_lib):
    assert ribbit_amd.ABI_SYMBOLS
    for name in ribbit_amd.ABI_SYMBOLS:
        assert getattr(hip_lib, name).argtypes is not None, f"{name} has no argtypes"


def test_failing_call_names_its_symbol(hip_lib):
    with pytest.raises(ribbit_amd.RibbitHipError) as e:
        ribbit_amd.host_record_loci(-1, [(0, 1)])
    assert str(e.value).startswith("ribbit_host_record_loci error -1: ")
    assert str(e.value) == "ribbit_host_record_loci error -1: " + hip_lib.ribbit_hip_last_error().decode()
    assert len(str(e.value)) > len("ribbit_host_record_loci error -1: ")


@pytest.mark.parametrize("builder,struct,cname", [(ribbit_amd.primer_params, ribbit_amd.PrimerParams, "RibbitPrimerParams"),
                                                  (ribbit_amd.primer_pair_params, ribbit_amd.PrimerPairParams, "RibbitPrimerPairParams"),
                                                  (ribbit_amd.product_params, ribbit_amd.ProductParams, "RibbitProductParams")])
def test_params_builders_refuse_bad_fields(builder, struct, cname):
    field = struct._fields_[0][0]
    assert isinstance(builder(), struct) and getattr(builder(**{field: 7}), field) == 7
    assert getattr(builder(**{field: -2**31}), field) == -2**31 and getattr(builder(**{field: 2**31 - 1}), field) == 2**31 - 1
    with pytest.raises(TypeError) as e:
        builder(no_such_field=1)
    assert str(e.value) == f"{cname} has no field 'no_such_field'"
    for value in (2**31, -2**31 - 1):
        with pytest.raises(ValueError) as e:
            builder(**{field: value})
        assert str(e.value) == f"{field} {value} does not fit int32"
