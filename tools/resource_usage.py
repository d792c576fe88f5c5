#!/usr/bin/env python3
"""Per-kernel register / spill / LDS / occupancy table of HIP translation units
for gfx950, from the compiler's kernel-resource-usage remarks (no GPU needed).

  python tools/resource_usage.py [--digest] [source.hip ...] [filter]

Several sources give one table; without a source: the path tracer's units
(RENDER_UNITS: tmpt_render.hip and the engines split off it).  --digest adds a column with a
digest of each kernel's code bytes (its symbol's range of .text in the unit's
device code object), so two builds can be compared kernel by kernel:

  python tools/resource_usage.py --digest | sort > after.txt

Compiles the device code with the library's own flags (csrc/Makefile; EXTRA in
the environment is appended) into a temporary directory, so a code change can
be checked for register pressure and spills before a GPU run."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toymeshpathtracer_amd", "csrc")
RENDER_UNITS = ("tmpt_mega.hip", "tmpt_hitscene.hip", "tmpt_wavefront.hip", "tmpt_rows.hip", "tmpt_render.hip",
                "tmpt_shadow.hip", "tmpt_query.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-gpu-flush-denormals-to-zero",
         f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "-O2", "-fno-slp-vectorize"]
KEYS = ("VGPRs", "AGPRs", "SGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]",
        "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def demangle(names):
    for tool in (os.path.join(LLVM_BIN, "llvm-cxxfilt"), "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True,
                                 check=True).stdout.splitlines()
            return [o.split("(")[0] for o in out]
        except Exception:
            continue
    return names


def code_digests(obj):
    """{mangled kernel name: digest of its code bytes} of a device code object."""
    readelf = os.path.join(LLVM_BIN, "llvm-readelf")
    text = None
    for line in subprocess.run([readelf, "-SW", obj], capture_output=True, text=True, check=True).stdout.splitlines():
        p = line.replace("[", " ").replace("]", " ").split()
        if len(p) > 5 and p[1] == ".text":
            text = (int(p[3], 16), int(p[4], 16))  # address, file offset
    data = open(obj, "rb").read()
    out = {}
    for line in subprocess.run([readelf, "-sW", obj], capture_output=True, text=True, check=True).stdout.splitlines():
        p = line.split()
        if len(p) >= 8 and p[3] == "FUNC":
            off = int(p[1], 16) - text[0] + text[1]
            out[p[7]] = hashlib.sha256(data[off:off + int(p[2])]).hexdigest()[:12]
    return out


def unit_rows(src, obj, extra):
    r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, "-x", "hip", "--cuda-device-only",
                        "--no-gpu-bundle-output", "-c", src, "-o", obj, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        sys.exit(r.returncode)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (.*?): (.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2).strip()
        if k == "Function Name":
            cur = {"name": v}
            rows.append(cur)
        elif cur is not None and k in KEYS:
            cur[k] = v
    return rows


def main():
    args = sys.argv[1:]
    digest = "--digest" in args
    args = [a for a in args if a != "--digest"]
    srcs = [a for a in args if os.path.isfile(a)]
    filt = next((a for a in args if not os.path.isfile(a)), "")
    if not srcs:
        srcs = [os.path.join(CSRC, u) for u in RENDER_UNITS]
    extra = os.environ.get("EXTRA", "").split()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, src in enumerate(srcs):
            obj = os.path.join(tmp, f"unit{i}.co")
            unit = unit_rows(src, obj, extra)
            if digest:
                d = code_digests(obj)
                for x in unit:
                    x["digest"] = d.get(x["name"], "?")
            rows += unit
    names = demangle([x["name"] for x in rows])
    print(f"{'kernel':<100} {'VGPR':>5} {'SGPR':>5} {'vspill':>6} {'sspill':>6} {'scratch':>7} {'occ':>4} {'LDS':>6}"
          + (f" {'code':>12}" if digest else ""))
    for x, n in zip(rows, names):
        if filt and filt not in n:
            continue
        print(f"{n[:100]:<100} {x.get('VGPRs', '?'):>5} {x.get('TotalSGPRs', x.get('SGPRs', '?')):>5} {x.get('VGPRs Spill', '?'):>6} "
              f"{x.get('SGPRs Spill', '?'):>6} {x.get('ScratchSize [bytes/lane]', '?'):>7} "
              f"{x.get('Occupancy [waves/SIMD]', '?'):>4} {x.get('LDS Size [bytes/block]', '?'):>6}"
              + (f" {x['digest']:>12}" if digest else ""))


if __name__ == "__main__":
    main()
