"""The layering of tests/ ("Layout of the tests"): no module of tests/ or profiles/ imports a test module, and every helper and
multi-rank worker of tests/ imports on a CPU -- a worker's broken import would otherwise show only inside a child process on the GPU."""
import ast
import glob
import importlib
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_module_imports_a_test_module():
    bad = []
    for path in glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True) + glob.glob(os.path.join(ROOT, "profiles", "**", "*.py"), recursive=True):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad += ["%s:%d imports %s" % (os.path.relpath(path, ROOT), node.lineno, n) for n in names if n.split(".")[-1].startswith("test_")]
    assert not bad, "\n".join(bad)


def test_helper_modules_and_workers_import():
    names = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(ROOT, "tests", "*.py")))
    names = [n for n in names if not n.startswith("test_") and n != "conftest"]
    assert "common" in names and "mr_gpu_tidal" in names, names
    for n in names:
        importlib.import_module(n)
