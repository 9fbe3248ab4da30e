"""CPU tests of the layout of tests/: what tests share lives in plain modules (batch_support.py, update_checks.py, ...), never in
a test module.  No file of tests/ or tools/ imports a test_*.py module; no plain module of tests/ defines a test or a fixture
(pytest would not collect the one nor find the other); the plain modules' imports of each other form no cycle, so any of them
imports alone; and batch_support.instance_seed gives the values of the two spellings it replaced.  The bench tools of tools/ are
held the same way: none imports a *_bench module, what they share is tools/bench_support.py, which imports no other file of tools/
and reaches torch only inside functions.  Sources are read as text and ASTs; nothing of the GPU side is touched."""
import ast
import glob
import os

import numpy as np

from batch_support import instance_seed

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def _tree(path):
    with open(path) as f:
        return ast.parse(f.read(), path)


def _imported(tree):
    """(module name, line) of every import statement, at any nesting depth"""
    out = []
    for n in ast.walk(tree):
        if isinstance(n, ast.Import):
            out += [(a.name, n.lineno) for a in n.names]
        elif isinstance(n, ast.ImportFrom) and n.module:
            out.append((n.module, n.lineno))
    return out


def _plain_modules():
    """the modules directly under tests/ that pytest does not collect, by name (conftest.py is pytest's own)"""
    names = [os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TESTS, "*.py"))]
    return sorted(n for n in names if not n.startswith("test_") and n != "conftest")


def _is_fixture(dec):
    d = dec.func if isinstance(dec, ast.Call) else dec
    return (d.attr if isinstance(d, ast.Attribute) else getattr(d, "id", "")) == "fixture"


def test_no_file_imports_a_test_module():
    files = glob.glob(os.path.join(TESTS, "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))
    assert len(files) > 50
    bad = [(os.path.relpath(f, ROOT), line, mod) for f in sorted(files) for mod, line in _imported(_tree(f))
           if mod.split(".")[-1].startswith("test_")]
    assert not bad, bad


def test_no_tool_imports_a_bench_tool_and_bench_support_imports_no_tool():
    tools = sorted(glob.glob(os.path.join(ROOT, "tools", "*.py")))
    names = {os.path.basename(f)[:-3] for f in tools}
    assert "bench_support" in names and len([n for n in names if n.endswith("_bench")]) == 13
    bad = [(os.path.relpath(f, ROOT), line, mod) for f in tools for mod, line in _imported(_tree(f))
           if mod.split(".")[-1].endswith("_bench")]
    assert not bad, bad
    support = _tree(os.path.join(ROOT, "tools", "bench_support.py"))
    assert not [mod for mod, _ in _imported(support) if mod.split(".")[0] in names]
    # (torch only inside functions: nothing that runs when the module is imported reaches it)
    in_function = {id(n) for f in ast.walk(support) if isinstance(f, (ast.FunctionDef, ast.AsyncFunctionDef)) for n in ast.walk(f)}
    torch_lines = [(line, id(n) in in_function) for n in ast.walk(support) if isinstance(n, (ast.Import, ast.ImportFrom))
                   for mod, line in _imported(n) if mod.split(".")[0] == "torch"]
    assert torch_lines and all(inside for _, inside in torch_lines), torch_lines


def test_plain_modules_define_no_test_and_no_fixture():
    bad = []
    for name in _plain_modules():
        for n in ast.walk(_tree(os.path.join(TESTS, name + ".py"))):
            if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)):
                if n.name.startswith("test_") or any(_is_fixture(d) for d in n.decorator_list):
                    bad.append((name, n.lineno, n.name))
    assert not bad, bad


def test_plain_modules_import_each_other_without_a_cycle():
    plain = _plain_modules()
    assert {"helpers", "batch_support", "update_checks", "obstacle_cases", "fleet_support", "costmap_support", "grid_cases",
            "resident_loops"} <= set(plain)
    uses = {m: sorted({mod for mod, _ in _imported(_tree(os.path.join(TESTS, m + ".py"))) if mod in plain}) for m in plain}
    done, cycles = set(), []

    def visit(m, trail):
        if m in trail:
            cycles.append(trail[trail.index(m):] + [m])
        elif m not in done:
            for u in uses[m]:
                visit(u, trail + [m])
            done.add(m)

    for m in plain:
        visit(m, [])
    assert not cycles, cycles


def test_instance_seed_is_both_spellings_it_replaced():
    """the masked Python integer, and the wrapping uint64 array product (b + 1) * c that two fleet tests wrote (salt 0 only)"""
    c = 0x9E3779B97F4A7C15
    bs = np.arange(64, dtype=np.uint64)
    product = (bs + np.uint64(1)) * np.uint64(c)
    for salt in (0, 1, 3):
        masked = [(c * (b + 1) + salt) & 0xFFFFFFFFFFFFFFFF for b in range(64)]
        assert [instance_seed(b, salt) for b in range(64)] == masked, salt
        assert (np.array(masked, dtype=np.uint64) == product + np.uint64(salt)).all(), salt
    assert [instance_seed(b) for b in range(64)] == [int(x) for x in product]
