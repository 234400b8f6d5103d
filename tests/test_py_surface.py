"""The Python surface of crdts_hip, pinned: every public name, the kind and
signature of every function and class member, and the value of every int /
str / tuple / dict constant recorded in tests/golden/py_surface.json must
still be offered (new names are allowed; missing or changed ones fail).

    python tests/test_py_surface.py --write     # re-record the fixture
"""
import importlib
import inspect
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "py_surface.json")
ALIASES = ("C", "np", "os")  # bare third-party module aliases, not part of the surface
SUBMODULES = ("_lib", "record", "replica", "lwwreg", "clock_bincode", "ops_bincode")


def _dunder(name):
    return name.startswith("__") and name.endswith("__")


def _plain(v):
    """JSON form of an int / str / tuple / dict constant (tuples as lists,
    dict keys as strings), None for anything else."""
    if isinstance(v, bool) or v is None:
        return None
    if isinstance(v, str) and os.path.isabs(v):
        return None  # (a path of this checkout, LIB_PATH: not a property of the package)
    if isinstance(v, (int, str)):
        return v
    if isinstance(v, tuple):
        items = [_plain(x) for x in v]
        return None if any(x is None for x in items) else items
    if isinstance(v, dict):
        items = {str(k): _plain(x) for k, x in v.items()}
        return None if any(x is None for x in items.values()) else items
    return None


def _signature(obj):
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):
        return None


def _member(cls, name):
    static = inspect.getattr_static(cls, name)
    if isinstance(static, staticmethod):
        kind = "staticmethod"
    elif isinstance(static, classmethod):
        kind = "classmethod"
    elif isinstance(static, property):
        kind = "property"
    elif isinstance(static, types.FunctionType):
        kind = "function"
    else:
        kind = "constant"
    rec = {"kind": kind}
    if kind in ("function", "classmethod", "staticmethod"):
        rec["signature"] = _signature(getattr(cls, name))
    elif kind == "constant":
        v = _plain(static)
        if v is not None:
            rec["value"] = v
    return rec


def snapshot():
    import crdts_hip

    out = {}
    for name in dir(crdts_hip):
        if _dunder(name) or name in ALIASES:
            continue
        obj = getattr(crdts_hip, name)
        if inspect.isclass(obj):
            names = [n for n, _ in inspect.getmembers(obj) if not _dunder(n)] + ["__init__"]
            out[name] = {"kind": "class", "members": {n: _member(obj, n) for n in names}}
        elif inspect.isfunction(obj):
            out[name] = {"kind": "function", "signature": _signature(obj)}
        elif inspect.ismodule(obj):
            out[name] = {"kind": "module"}
        else:
            rec = {"kind": "constant"}
            v = _plain(obj)
            if v is not None:
                rec["value"] = v
            out[name] = rec
    return out


def test_surface_offers_what_the_fixture_records():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = snapshot()
    bad = []
    for name, w in want.items():
        g = got.get(name)
        if g is None:
            bad.append(f"{name}: missing")
            continue
        if w["kind"] != "class":
            if g != w:
                bad.append(f"{name}: {g} != {w}")
            continue
        if g["kind"] != "class":
            bad.append(f"{name}: no longer a class")
            continue
        for m, wm in w["members"].items():
            gm = g["members"].get(m)
            if gm != wm:
                bad.append(f"{name}.{m}: {gm} != {wm}")
    assert not bad, "\n".join(bad)


def test_fixture_size():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want) == 73  # (76 names with the three module aliases, which are not recorded)
    assert sum(len(w["members"]) for w in want.values() if w["kind"] == "class") == 342


def test_all_names_exist():
    import crdts_hip

    missing = [n for n in crdts_hip.__all__ if not hasattr(crdts_hip, n)]
    assert not missing
    for n in ("MapSlab", "MapOrswotSlab", "MapOrswotOps", "MapMapSlab", "OrswotOps"):
        assert n in crdts_hip.__all__


def test_submodules_import():
    for m in SUBMODULES:
        importlib.import_module("crdts_hip." + m)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "rust-crdt_amd"))
    if sys.argv[1:] == ["--write"]:
        snap = snapshot()
        with open(GOLDEN, "w") as f:
            json.dump(snap, f, indent=0, sort_keys=True)
            f.write("\n")
        print(len(snap), "names,", sum(len(w["members"]) for w in snap.values() if w["kind"] == "class"), "members")
