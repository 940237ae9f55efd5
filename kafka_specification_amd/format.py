"""Canonical-byte states as TLA+ values, the way TLC prints a trace state (`/\\ var = value`) [TLC-recall]: the library's
kmc_format_state (csrc/kmc_frontend.cpp), which the native command line prints with too.  The byte layout: include/kmc.h."""
from __future__ import annotations

import ctypes as C

from . import _native as nat


def format_state(cfg, b: bytes) -> str:
    c = cfg.to_native()
    raw = (C.c_uint8 * len(b)).from_buffer_copy(b)
    n = nat.lib().kmc_format_state(C.byref(c), raw, len(b), None, 0)
    if n < 0:
        raise ValueError(nat.lib().kmc_last_error().decode("utf-8", "replace"))
    out = C.create_string_buffer(n + 1)
    nat.lib().kmc_format_state(C.byref(c), raw, len(b), out, n + 1)
    return out.value.decode()
