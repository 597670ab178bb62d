"""The host-side plan answers of the conv library against tests/golden/igemm_plan_table.json, recorded from the libraries of
the commit before conv_igemm.hip's host dispatch was rewritten (tests/golden/make_igemm_plan_table.py says what a row holds):
every plan-time question must be answered as it was, in the product library and under the tuning library's switches.
No device needed: nothing is launched and no row reaches the occupancy query."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def table():
    spec = importlib.util.spec_from_file_location("make_igemm_plan_table", os.path.join(GOLDEN, "make_igemm_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert os.path.getsize(mod.FIXTURE) < 200 * 1024
    with open(mod.FIXTURE) as f:
        return mod, json.load(f)


def test_the_rows_are_the_shape_tables_of_the_suite(table):
    mod, want = table
    shapes = mod.shapes()
    assert [key for key, _ in want["rows"]] == [key for key, _ in shapes]
    assert [[r[0] for r in rows] for _, rows in want["rows"]] == [[list(r) for r in rows] for _, rows in shapes]
    assert list(want["tuning"]) == [name for name, _ in mod.TUNING_CONFIGS]
    keys = {key.split()[0] for key, _ in shapes}
    assert keys == {"inception", "stem", "head", "toy"} and sum(key.startswith("inception") for key, _ in shapes) == 2 * 65
    assert any(r[-1] == 8 for _, rows in shapes for r in rows) and any(r[-1] == 4 for _, rows in shapes for r in rows)


def test_product_library_answers_as_recorded(table):
    mod, want = table
    from tumblr_emotions_amd import _lib
    got = mod.product_rows(_lib.load())
    for (key, g), (_, w) in zip(got, want["rows"]):
        for grow, wrow in zip(g, w):
            assert grow == wrow, (key, grow[0])
    assert got == want["rows"]


def test_tuning_library_answers_as_recorded_under_its_switches(table):
    mod, want = table
    from tumblr_emotions_amd import _lib
    got = mod.tuning_digests(_lib.load_tuning())
    keys = [key for key, _ in mod.shapes()]
    for name, digests in want["tuning"].items():
        differ = [k for k, g, w in zip(keys, got[name], digests) if g != w]
        assert not differ, (name, differ[:8])
    assert got == want["tuning"]
    # the switches are back at their defaults: the tuning library answers like the product again
    assert mod.tuning_digests.__doc__ and got["default"] == [mod.digest([mod.answers(_lib.load_tuning(), r) for r in rows])
                                                              for _, rows in mod.shapes()]
