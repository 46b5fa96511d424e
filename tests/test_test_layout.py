"""CPU: the layout of tests/ itself.  Shared helpers live in the *_common.py modules; a test module never imports another test
module (running one file would import, and assert-rewrite, the others), and the two helpers every device test uses - `bits`
(float64 as uint64) and `strip` (records without the running-return words) - have one definition, so one meaning."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_no_test_module_is_imported_and_bits_and_strip_are_defined_once():
    trees = {os.path.basename(f): ast.parse(open(f).read(), f) for f in sorted(glob.glob(os.path.join(HERE, "*.py")))}
    assert len(trees) > 40
    imports, homes = [], {"bits": [], "strip": []}
    for name, tree in trees.items():
        for node in ast.walk(tree):                       # (module level and nested in functions alike)
            if isinstance(node, ast.Import):
                imports += [(name, node.lineno, a.name) for a in node.names]
            elif isinstance(node, ast.ImportFrom):
                imports.append((name, node.lineno, node.module or ""))
            elif isinstance(node, ast.FunctionDef) and node.name in homes:
                homes[node.name].append(name)
    bad = [f"{name}:{line} imports {mod}" for name, line, mod in imports if mod.split(".")[-1].startswith("test_")]
    assert not bad, bad
    assert homes == {"bits": ["vec_common.py"], "strip": ["vec_common.py"]}, homes
