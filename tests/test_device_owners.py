"""Who may allocate, read as text (no compiler, no GPU): device memory, pinned
memory, events and streams are made and released by the owner types of
csrc/tmpt_device.h and by nothing else under csrc/, the device's free memory is
asked for there alone (free_budget), and tmpt_scene_destroy releases no member
by hand -- `delete h` does, through the owners Scene is made of."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toymeshpathtracer_amd", "csrc")
OWNERS = "tmpt_device.h"

#: the HIP calls only tmpt_device.h may name (a word's prefix: hipMalloc also
#: finds hipMallocAsync, hipEventCreate also hipEventCreateWithFlags, ...)
CALLS = ("hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipEventCreate", "hipEventDestroy",
         "hipStreamCreate", "hipStreamDestroy", "hipMemGetInfo")
CALL_RE = re.compile(r"\b(" + "|".join(CALLS) + r")\w*")

DESTROY_MAX_LINES = 15


def sources():
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".cpp")))
    assert OWNERS in names and "tmpt_api.cpp" in names and "tmpt_cli.cpp" in names
    return names


def test_only_the_owners_header_allocates():
    found = []
    for name in sources():
        if name == OWNERS:
            continue
        for no, line in enumerate(open(os.path.join(CSRC, name)), 1):
            for m in CALL_RE.finditer(line):
                found.append(f"{name}:{no}: {m.group(0)}")
    assert not found, "outside tmpt_device.h:\n" + "\n".join(found)


def test_the_owners_header_has_every_call():
    """The list above is the header's own: each call occurs there, so a renamed or
    dropped one does not leave the first test checking for a word nobody writes."""
    text = open(os.path.join(CSRC, OWNERS)).read()
    missing = [c for c in CALLS if not re.search(rf"\b{c}", text)]
    assert not missing, missing


def function_body(text, name):
    m = re.search(rf"^int {name}\([^)]*\)\s*\{{", text, re.M)
    assert m, f"no definition of {name}"
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def test_scene_destroy_releases_no_member_by_hand():
    body = function_body(open(os.path.join(CSRC, "tmpt_api.cpp")).read(), "tmpt_scene_destroy")
    lines = [ln for ln in body.splitlines() if ln.strip()]
    assert len(lines) <= DESTROY_MAX_LINES, f"tmpt_scene_destroy has {len(lines)} lines"
    assert "delete h;" in body
    assert "hipSetDevice" in body and "hipStreamSynchronize" in body  # it still waits for the scene's streams
    assert not re.search(r"\.reset\(\)", body), "a member released by hand"
