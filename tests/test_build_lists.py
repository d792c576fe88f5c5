"""The build's file lists, read as text (no compiler, no GPU): every HIP unit and
header under csrc/ is named in the Makefile, and the units whose kernels
tools/resource_usage.py tabulates by default (RENDER_UNITS) exist and are built,
so a new unit is not silently left out of the library or of the digest table."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toymeshpathtracer_amd", "csrc")


def make_list(name):
    """The words of the Makefile variable `name` (':=' assignment, '\\' continuations)."""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(rf"^{name}\s*:=(.*)$", text, re.M)
    assert m, f"Makefile: no {name} := line"
    return m.group(1).split()


def render_units():
    tree = ast.parse(open(os.path.join(ROOT, "tools", "resource_usage.py")).read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "RENDER_UNITS" for t in node.targets):
            return list(ast.literal_eval(node.value))
    raise AssertionError("tools/resource_usage.py: no RENDER_UNITS")


def test_every_hip_unit_is_built():
    units = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert units
    missing = [u for u in units if u not in make_list("SRCS_HIP")]
    assert not missing, f"not in the Makefile's SRCS_HIP: {missing}"


def test_every_header_is_a_dependency():
    headers = sorted(f for f in os.listdir(CSRC) if re.fullmatch(r"tmpt_.*\.h", f))
    assert headers
    missing = [h for h in headers if h not in make_list("HDRS")]
    assert not missing, f"not in the Makefile's HDRS: {missing}"


def test_render_units_exist_and_are_built():
    units = render_units()
    assert units
    srcs = make_list("SRCS_HIP")
    for u in units:
        assert os.path.isfile(os.path.join(CSRC, u)), f"RENDER_UNITS: {u} does not exist"
        assert u in srcs, f"RENDER_UNITS: {u} is not in the Makefile's SRCS_HIP"
