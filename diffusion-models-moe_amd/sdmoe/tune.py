"""The library's tuning knobs by name (include/sdmoe.h defines them). Names, ids, defaults and values are read from the
library's own table, so nothing here or in a caller restates them.

    with tune.tuned(ksplit=4, halo=0):   # set, and put back what was set before on the way out
        ...
"""
from __future__ import annotations

import contextlib

from . import _lib


def knobs() -> dict:
    """{name: (id, default, value)} of every knob, as the library reports them now."""
    return {name: (kid, default, value) for kid, name, default, value in _lib.knob_table()}


def parse(spec: str) -> dict:
    """An SDMOE_TUNE-style "knob=value,..." string, knobs by id or name (_lib.parse_tune) -> {name: value}."""
    names = {kid: name for name, (kid, _, _) in knobs().items()}
    pairs = _lib.parse_tune(spec)
    for kid, _ in pairs:
        if kid not in names:
            raise _lib.SdmoeError(f"no knob with id {kid} (known: {', '.join(map(str, names))})")
    return {names[kid]: value for kid, value in pairs}


def set(**by_name) -> None:
    """Set knobs by name; an unknown name or an illegal value raises SdmoeError (the knob then keeps its value)."""
    table = knobs()
    for name in by_name:
        if name not in table:
            raise _lib.SdmoeError(f"no knob named {name!r} (known: {', '.join(table)})")
    lib = _lib.load()
    for name, value in by_name.items():
        _lib.check(lib.sdmoe_tune(table[name][0], value), f"sdmoe_tune({name}={value})")


def reset() -> None:
    """Every knob back to its default."""
    _lib.check(_lib.load().sdmoe_tune_reset(), "sdmoe_tune_reset")


@contextlib.contextmanager
def tuned(**by_name):
    """Set knobs by name for the block; afterwards, also on an exception, the values they had before (not the
    defaults: a run under SDMOE_TUNE keeps its setting). Nests."""
    table = knobs()
    before = {name: table[name][2] for name in by_name if name in table}
    try:
        set(**by_name)
        yield
    finally:
        set(**before)
