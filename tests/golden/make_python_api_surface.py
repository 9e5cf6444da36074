"""Generator of tests/golden/python_api_surface.json: the public surface of the Python package, as a record that
tests/test_python_api_cpu.py regenerates in memory and compares.  The committed file is the one generated at the commit
before the bindings moved onto binding.py, so the comparison says that the move changed no name, signature or constant.

For every module of the package:
  names      the sorted non-underscore module-level names the package itself gives meaning to -- functions and classes of
             the package (re-exports from a sibling module included) and plain values; imported modules and names from
             outside the package (typing, dataclasses, numpy, ...) are not the package's surface -- plus `_lib`, `_check`
             and `_rows` where the module has them
  functions  str(inspect.signature(f)) of every recorded function
  protos     the sorted keys of PROTOS / _PROTOS
  constants  the values of module-level int / float / str constants (a tuple of those as a list)
  classes    for every recorded class, the module that defines it and its non-underscore members plus __init__ as dir()
             shows them, inherited ones included: the signature of a callable, "property" for a property, the value of an
             enum member.  Plain data attributes, base classes and docstrings are not recorded.

Importing the package needs neither the built library nor a device.

usage: python tests/golden/make_python_api_surface.py [dest_dir]
"""
import enum
import importlib
import inspect
import json
import os
import pkgutil
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PACKAGE = "the_algorithm_amd"
PRIVATE_KEPT = ("_lib", "_check", "_rows")


def _package():
    sys.path.insert(0, os.path.dirname(HERE))
    from _pkg import load_package

    return load_package()


def _signature(obj) -> str:
    try:
        return re.sub(r" at 0x[0-9a-f]+", "", str(inspect.signature(obj)))  # (a default that is a function: no address)
    except (TypeError, ValueError):
        return "<no signature>"


def _own(value) -> bool:
    return (getattr(value, "__module__", None) or "").startswith(PACKAGE)


def _class_record(cls) -> dict:
    members = {}
    for name in dir(cls):
        if name.startswith("_") and name != "__init__":
            continue
        raw = inspect.getattr_static(cls, name)
        if isinstance(raw, property):
            members[name] = "property"
        elif isinstance(raw, enum.Enum):
            members[name] = raw.value
        elif isinstance(raw, (staticmethod, classmethod)):
            members[name] = type(raw).__name__ + _signature(getattr(cls, name))
        elif callable(raw):
            members[name] = _signature(raw)
    return {"module": cls.__module__, "members": members}


def _constant(value):
    if isinstance(value, bool) or not isinstance(value, (int, float, str, tuple)):
        return None
    if isinstance(value, tuple):
        return list(value) if all(isinstance(x, (int, float, str)) and not isinstance(x, bool) for x in value) else None
    if isinstance(value, str) and value.startswith(ROOT):
        return "<root>" + value[len(ROOT):]  # a path into the checkout, wherever that lies
    return value


def _module_record(mod) -> dict:
    names, functions, classes, constants = [], {}, {}, {}
    for name, value in vars(mod).items():
        if name.startswith("_") and name not in PRIVATE_KEPT:
            continue
        if inspect.ismodule(value) or (name.startswith("_") and not inspect.isroutine(value)):
            continue  # (simclusters_ann._lib is the loaded library itself, or None before the first load)
        if inspect.isclass(value) or inspect.isroutine(value):
            if not _own(value):
                continue
            if inspect.isclass(value):
                classes[name] = _class_record(value)
            else:
                functions[name] = _signature(value)
        elif type(value).__module__ != "builtins" and not _own(type(value)):
            continue  # a typing alias, a __future__ feature, a compiled pattern ...
        else:
            c = _constant(value.value if isinstance(value, enum.Enum) else value)
            if c is not None:
                constants[name] = c
        names.append(name)
    protos = vars(mod).get("PROTOS", vars(mod).get("_PROTOS"))
    return {"names": sorted(names), "functions": functions, "classes": classes, "constants": constants,
            "protos": sorted(protos) if isinstance(protos, dict) else None}


def surface() -> dict:
    pkg = _package()
    out = {"__init__": _module_record(pkg)}
    for info in pkgutil.iter_modules(pkg.__path__):
        if not os.path.exists(os.path.join(pkg.__path__[0], info.name + ".py")):
            continue  # the built library beside the sources is no Python module
        out[info.name] = _module_record(importlib.import_module(f"{PACKAGE}.{info.name}"))
    return out


def dumps(record: dict) -> str:
    return json.dumps(record, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    dest = sys.argv[1] if len(sys.argv) > 1 else HERE
    with open(os.path.join(dest, "python_api_surface.json"), "w") as f:
        f.write(dumps(surface()))
