"""not gpu: the import rules of oracle/__init__.py.  The product never imports the oracle, the recording stand-in or the reference;
only the recorder touches the stand-in; the benchmark and the GPU tests never import the recorder."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STANDIN_NAMES = {"torch_geometric", "torch_scatter", "torch_sparse", "ogb", "_placeholder"}


def _imports(path):
    """Top-level names of every import statement of a Python file (relative imports excluded)."""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.level == 0 and node.module:
            names.add(node.module.split(".")[0])
    return names


def _python_files(*parts):
    top = os.path.join(ROOT, *parts)
    if os.path.isfile(top):
        return [top]
    return [os.path.join(d, f) for d, _, fs in os.walk(top) for f in fs if f.endswith(".py")]


def test_product_imports_neither_oracle_nor_standin():
    files = _python_files("dp_gsat_amd")
    assert len(files) > 10
    for path in files:
        bad = _imports(path) & ({"oracle", "tests"} | STANDIN_NAMES)
        assert not bad, f"{os.path.relpath(path, ROOT)} imports {sorted(bad)}"


def test_only_the_recorder_reaches_the_standin():
    """Nothing outside oracle/standin imports a stand-in name, except the recorder (inside its recording process) and the stand-in's
    own host test."""
    for path in _python_files("bench.py") + _python_files("__graft_entry__.py") + _python_files("examples") + _python_files("oracle") + _python_files("tests"):
        rel = os.path.relpath(path, ROOT)
        if rel.startswith(os.path.join("oracle", "standin")):
            continue
        if rel not in (os.path.join("tests", "test_ref_standin_host.py"), os.path.join("oracle", "record_reference.py")):
            bad = _imports(path) & STANDIN_NAMES
            assert not bad, f"{rel} imports {sorted(bad)}"


def test_gpu_tests_and_benchmark_do_not_import_the_recorder():
    for path in _python_files("bench.py") + _python_files("__graft_entry__.py") + [p for p in _python_files("tests") if os.path.basename(p).startswith("test_gpu")]:
        text = open(path).read()
        assert "record_reference" not in text.replace("oracle/record_reference.py", ""), os.path.relpath(path, ROOT)
