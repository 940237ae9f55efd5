"""Identity of the spec text the kernels were lowered from.

The command lines do not parse TLA+: they map the root module's NAME to a hand-lowered model.  A drop-in must not
silently check the stock model when the user has edited the spec, so both front ends hash the module they are given and
every module it EXTENDS / INSTANCEs (those found next to it) and compare with the revision of
hachikuji/kafka-specification the lowering was written against.  A mismatch is refused unless -force is given; a module
file that does not exist (this repository ships no copy of the reference's .tla files) is reported and the built-in
lowering is checked.

The table of hashes, the walk and the SHA-256 are the library's (csrc/kmc_frontend.cpp: kmc_spec_check); models/MCAsyncIsr.tla
is authored in this repository and hashed at run time against the copy in models/.
"""
from __future__ import annotations

import ctypes as C

from . import _native as nat

STATUS = ("ok", "absent", "mismatch")


def check_spec(path: str):
    """-> (status, messages).  status: "ok" every module of the closure that exists matches the lowered revision;
    "absent" the root module file does not exist; "mismatch" some module differs or is unknown."""
    msgs = C.create_string_buffer(16384)
    status = nat.lib().kmc_spec_check(path.encode(), msgs, len(msgs))
    return STATUS[status], msgs.value.decode("utf-8", "replace").splitlines()
