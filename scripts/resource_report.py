"""The compiler's gfx950 resource report of every kernel of the engine units
(hipcc -Rpass-analysis=kernel-resource-usage, build.py's flags), for this tree
and, with --before, for another checkout of the project (the parent commit):
which kernels exist on both sides, whether their figures are identical, and
the figures of the kernels whose names match --new.  The engine units of a
tree are those its build.py lists (ENGINE_UNITS; a checkout without the list
has engine.hip alone), reported as one set: a kernel that moved between
units compares equal, one that two units define is listed.  --ds-monoids
compares the ds_tu.hip units of those downsampling monoids as well, both
parts.

    python -m scripts.resource_report --before PATH/TO/PARENT/CHECKOUT \
        --new k_rr_ --out profiles/rollup_rows_resources.json
"""
import argparse
import importlib.util
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]",
          "Dynamic Stack", "Occupancy [waves/SIMD]", "SGPRs Spill",
          "VGPRs Spill", "LDS Size [bytes/block]")


def report(root, unit="engine.hip", defines=()):
    """{demangled kernel name: {field: value}} of one translation unit."""
    from opentsdb_amd import build
    src = os.path.join(root, "opentsdb_amd", "csrc", unit)
    cmd = [build.HIPCC] + build.FLAGS + ["-D" + d for d in defines] + [
        "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
        "-o", os.devnull, src]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, check=True)
    out, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: +([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and cur is not None and m.group(1).strip() in FIELDS:
            cur[m.group(1).strip()] = m.group(2).strip()
    names = sorted(out)
    dem = subprocess.run(["c++filt"] + names,
                         stdout=subprocess.PIPE, text=True).stdout.split("\n")
    return {d or n: out[n] for n, d in zip(names, dem)}


def engine_units(root):
    """The engine units' sources of the checkout at root."""
    spec = importlib.util.spec_from_file_location(
        "_otsdb_build_of_" + str(abs(hash(root))),
        os.path.join(root, "opentsdb_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not hasattr(mod, "ENGINE_UNITS"):
        return ["engine.hip"]
    return [mod.UNIT_FILES[k][0] for k in mod.ENGINE_UNITS]


def report_engine(root):
    """(the union of report() over root's engine units, the kernels more than
    one of them defines)."""
    out, twice = {}, []
    for unit in engine_units(root):
        for k, v in report(root, unit).items():
            if k in out:
                twice.append(k)
            out[k] = v
    return out, sorted(twice)


def compare(before, after):
    return {"kernels_before": len(before), "kernels_after": len(after),
            "kernels_only_before": sorted(set(before) - set(after)),
            "kernels_only_after": sorted(set(after) - set(before)),
            "kernels_with_other_figures": sorted(
                k for k in before if k in after and before[k] != after[k])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", default=None, help="the parent's checkout")
    ap.add_argument("--new", default="k_rr_",
                    help="substring of the new kernels' names")
    ap.add_argument("--ds-monoids", default="",
                    help="comma-separated OTSDB_DS_MONOID values")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ds = [("ds_tu.hip", ("OTSDB_DS_MONOID=" + m, "OTSDB_DS_PART=%d" % part))
          for m in filter(None, a.ds_monoids.split(",")) for part in (1, 0)]
    after, twice = report_engine(ROOT)
    doc = {"arch": "gfx950",
           "source": "hipcc " + " ".join(__import__(
               "opentsdb_amd.build", fromlist=["FLAGS"]).FLAGS[1:5]) +
           " -Rpass-analysis=kernel-resource-usage, one translation unit per "
           "entry below; before = the parent commit",
           "new": {k: v for k, v in after.items() if a.new in k}}
    if a.before:
        before, _ = report_engine(a.before)
        old = {k: v for k, v in after.items() if a.new not in k}
        doc["engine units"] = dict(
            compare(before, old), units_before=engine_units(a.before),
            units_after=engine_units(ROOT), kernels_in_several_units=twice)
        for unit, d in sorted(ds):
            doc[unit + " " + " ".join("-D" + x for x in d)] = compare(
                report(a.before, unit, d), report(ROOT, unit, d))
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
