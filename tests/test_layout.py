"""The layout of tests/: what test modules share lives in plain helper modules, never in another test module."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_no_module_imports_a_test_module():
    bad = []
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        for node in ast.walk(ast.parse(open(path).read(), path)):
            names = [a.name for a in node.names] if isinstance(node, ast.Import) else [node.module or ""] if isinstance(node, ast.ImportFrom) else []
            bad += ["%s:%d imports %s" % (os.path.basename(path), node.lineno, n) for n in names if n.split(".")[0].startswith("test_")]
    assert not bad, bad
