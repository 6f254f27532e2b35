"""The stage plan (csrc/stage_plan.hip) answers what the routing it replaced answered: the two queries -- which touch no
device -- over the full product of blocks, reconstructions, dust, tasks, defer_finish and the eight path-selection
switches of artemis_hip_stage_general (scripts/stage_plan_table.py), held against tests/golden/stage_plan_table.json,
which that script recorded from a build of the commit before the plan existed."""
import importlib.util
import itertools
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("stage_plan_table", os.path.join(ROOT, "scripts", "stage_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def lib():
    """The library with the eight switches cleared for the sweep and put back afterwards."""
    from artemis_amd import capi
    L = capi.load()
    names = [n.encode() for n in _script().SWITCHES[1:]]
    before = {n: L.artemis_hip_get_option(n) for n in names}
    assert all(v >= 0 for v in before.values()), before  # (every switch is one the library knows)
    for n in names:
        L.artemis_hip_set_option(n, 0)
    yield L
    for n, v in before.items():
        L.artemis_hip_set_option(n, v)


def test_every_answer_of_the_two_queries_is_the_recorded_one(lib):
    from artemis_amd import capi
    T = _script()
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "stage_plan_table.json")))
    assert gold["axes"] == [name for name, _ in T.AXES]
    for name, values in T.AXES:
        assert gold[name] == values, name
    rows = list(itertools.product(*(values for _, values in T.AXES)))
    assert len(rows) == 9 * 10 * 3 * 8 * 10 * 3 and len(gold["answers"]) == len(rows)
    got = T.sweep(lib, capi)
    assert len(got) == len(rows)
    wrong = [(row, T.decode(g), T.decode(w)) for row, g, w in zip(rows, got, gold["answers"]) if g != w]
    assert not wrong, "%d rows differ; (row, (gas, dust) answered, recorded): %s" % (len(wrong), wrong[:10])
    for n in T.SWITCHES[1:]:
        assert lib.artemis_hip_get_option(n.encode()) == 0, n  # (the sweep clears what it sets)


def test_the_table_exercises_every_kernel_and_every_switch():
    """(of the recorded table alone: a sweep that never reached a kernel, or a switch that changed no row, would pin nothing)"""
    T = _script()
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "stage_plan_table.json")))
    pairs = {T.decode(c) for c in gold["answers"]}
    assert {g for g, _ in pairs} == {0, 1, 2, 3, 4} and {d for _, d in pairs} == {-1, 0, 1, 3, 5}
    n = len(gold["answers"]) // len(T.SWITCHES)
    base = gold["answers"][:n]
    for s, name in enumerate(T.SWITCHES[1:], 1):
        assert gold["answers"][s * n:(s + 1) * n] != base, name
