"""build.py's table of translation units against the sources: every unit's row
is exactly what its source includes, every csrc file belongs to a unit, and
the storage-row and histogram kernels are no longer engine.hip's."""
import os
import re

from opentsdb_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"')


def _includes(path, part):
    """The quoted csrc includes of one file.  ds_tu.hip's one conditional
    include (`#if OTSDB_DS_PART == 1` ... `#endif`) is taken for part 1 only;
    no other csrc include stands under a condition that differs between
    units."""
    out, skip = [], False
    with open(path) as f:
        for line in f:
            if re.match(r"\s*#\s*if\s+OTSDB_DS_PART\s*==\s*1\b", line):
                skip = part != 1
            elif skip and re.match(r"\s*#\s*endif\b", line):
                skip = False
            m = INCLUDE.match(line)
            if m and not skip and "/" not in m.group(1):
                out.append(m.group(1))
    return out


def closure(source, part=1):
    seen, todo = {source}, [source]
    while todo:
        for n in _includes(os.path.join(build.CSRC, todo.pop()), part):
            if n not in seen:
                seen.add(n)
                todo.append(n)
    return seen


PARTS = {"ds": 0, "cells": 1}


def test_every_row_is_its_units_include_closure():
    for kind, files in build.UNIT_FILES.items():
        assert len(set(files)) == len(files), kind
        assert set(files) == closure(files[0], PARTS.get(kind, 1)), kind
    # the two ds_tu.hip rows differ by the cells fold alone
    assert (set(build.UNIT_FILES["cells"]) - set(build.UNIT_FILES["ds"]) ==
            {"cellfold.hip"})


def test_every_csrc_file_belongs_to_a_unit():
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".h"))}
    listed = set().union(*build.UNIT_FILES.values())
    assert on_disk == listed
    assert on_disk | {"otsdb_agg.h"} == {os.path.basename(d) for d in build.DEPS}


def test_units_list_the_engine_units_first():
    units = build._units(build.OUT_DIR, ())
    n = len(build.ENGINE_UNITS)
    assert [u[3] for u in units[:n]] == list(build.ENGINE_UNITS)
    assert [os.path.basename(u[0]) for u in units[:n]] == [
        "engine.hip", "engine_rows.hip", "engine_hist.hip"]
    objs = [u[2] for u in units]
    assert len(set(objs)) == len(objs) == 4 + 2 * build.N_DS_MONOIDS
    assert all(u[3] in build.UNIT_FILES and
               os.path.basename(u[0]) == build.UNIT_FILES[u[3]][0]
               for u in units)


def test_engine_no_longer_includes_the_row_and_histogram_kernels():
    eng = closure("engine.hip")
    assert not eng & {"rows.hip", "rollup_rows.hip", "hist.hip", "histplan.h"}
    assert {"rows.hip", "rollup_rows.hip"} <= closure("engine_rows.hip")
    assert {"hist.hip", "histplan.h"} <= closure("engine_hist.hip")
