"""The option table (veritasfi_amd/csrc/vf_options.h), row by row, on the CPU: a host-compiled driver (tests/option_table_driver.py, UBSan)
sets every option on fresh defaults.  For each row: the default, both edges of what it accepts stored, one value past each edge and every
hole refused with the message the library has always given (option_table_driver.rows holds the literal texts), the value left alone by a
refusal; an unknown name refused as such; and a default-constructed RouteIn (vf_route.h) carrying the table's defaults.  Both builds:
the product's and -DVF_EXPERIMENTS (where the 4-wave form of k_scan_wide8 exists and its option accepts 4).  No GPU."""
import pytest

import option_table_driver as drv


@pytest.fixture(scope="module", params=[False, True], ids=["product", "experiments"])
def table(request, tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("option_table"), experiments=request.param), drv.rows(experiments=request.param)


def test_defaults_are_the_tables_in_options_and_in_route_in(table):
    exe, rows = table
    got = drv.defaults(exe)
    print(got)
    assert [name for name, _, _ in got] == [r[0] for r in rows]   # the same options, none missing on either side
    assert got == [(name, dflt, dflt) for name, dflt, _, _, _ in rows]


def test_edges_are_stored_and_values_past_them_and_holes_refused_with_the_message(table):
    exe, rows = table
    accept = [(name, v) for name, _, ok, _, _ in rows for v in ok]
    refuse = [(name, v, dflt, msg) for name, dflt, _, bad, msg in rows for v in bad]
    got = drv.set_each(exe, accept)
    wrong = [(n, v, g) for (n, v), g in zip(accept, got) if g != (drv.STORED, v, "")]
    assert not wrong, "not stored: %r" % wrong
    got = drv.set_each(exe, [(n, v) for n, v, _, _ in refuse])
    wrong = [(n, v, g) for (n, v, dflt, msg), g in zip(refuse, got) if g != (drv.REFUSED, dflt, msg)]
    assert not wrong, "not refused with the message and the value left alone: %r" % wrong
    assert all(bad for _, _, _, bad, _ in rows[:-1]) and rows[-1][0] == "debug"   # every checked row was tried past its edges


def test_unknown_names_are_refused_as_unknown(table):
    exe, _ = table
    names = ["no_such_option", "force_pat", "force_path_", "reserve_rows", "profile"]   # (the last two are the handle's actions, not rows)
    got = drv.set_each(exe, [(n, 1) for n in names])
    assert got == [(drv.UNKNOWN, 0, drv.UNKNOWN_MESSAGE % n) for n in names]
