"""Every row of `abi.UNITS` against its headers, the built library and a C compiler (the checks of tests/abi_checks.py), and the rows against
each other: no symbol in two units, every `ctypes.Structure` of abi.py in exactly one header.  What is particular to a unit (its refusals, its
kernels' budgets, its enums) is in that unit's tests/test_*_abi.py.  No GPU needed."""
import ctypes as C
import inspect
import itertools
import os

import pytest

from extended_legged_gym_amd import abi
from tests import abi_checks


def test_the_table_has_one_row_per_declare_function():
    declare = {name: fn for name, fn in inspect.getmembers(abi, inspect.isfunction) if name.startswith("declare_")}
    assert {"declare_" + unit: row.declare for unit, row in abi.UNITS.items()} == declare
    headers = [h for row in abi.UNITS.values() for h in row.headers]
    assert sorted(headers) == sorted(set(headers)) == sorted(f for f in os.listdir(abi_checks.INCLUDE) if f.endswith(".h"))


@pytest.mark.parametrize("unit", list(abi.UNITS))
def test_unit_agrees_with_its_headers_the_library_and_the_c_compiler(unit, tmp_path):
    abi_checks.check_unit_agreement(unit)
    abi_checks.check_struct_layouts(unit, tmp_path)


def test_units_are_pairwise_disjoint_and_every_struct_has_one_header():
    for a, b in itertools.combinations(abi.UNITS, 2):
        assert not set(abi.symbols(a)) & set(abi.symbols(b)), (a, b, sorted(set(abi.symbols(a)) & set(abi.symbols(b))))
    typedefs = [n for unit in abi.UNITS for n in abi_checks.header_structs(*abi.UNITS[unit].headers)]
    mirrors = [n for n, cls in inspect.getmembers(abi, inspect.isclass) if issubclass(cls, C.Structure) and cls is not C.Structure]
    assert sorted(typedefs) == sorted(mirrors) and len(typedefs) == len(set(typedefs))


def test_declare_sets_the_named_units_each_once(monkeypatch):
    lib = abi_checks.library()
    assert abi.declare(lib, "runner") is lib and lib.lg_obsnorm_step.argtypes is not None and lib.lg_mlp_forward.argtypes is None
    calls, real = [], abi.UNITS["runner"].declare
    monkeypatch.setitem(abi.UNITS, "runner", abi.UNITS["runner"]._replace(declare=lambda target: (calls.append(target), real(target))[1]))
    abi.declare(lib, "runner", "policy")
    assert lib not in calls and lib.lg_mlp_forward.argtypes is not None          # "runner" was set before; "policy" is new
    abi.declare(lib, *abi.UNITS)
    assert all(getattr(lib, sym).argtypes is not None for unit in abi.UNITS for sym in abi.symbols(unit)) and lib not in calls
    other = abi_checks.library("runner")
    assert calls.count(other) == 1 and abi.declare(other) is other and other.lg_mlp_forward.argtypes is None          # none named: none set
