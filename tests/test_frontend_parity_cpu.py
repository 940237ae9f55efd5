"""The one reader of .cfg files and printer of states (csrc/kmc_frontend.cpp, which both command lines ask) against what the Python
front end it replaced answered: tests/golden/frontend_parity.json was recorded from cfg.py / format.py of the commit before
the move (tests/golden/make_frontend_parity.py) — every shipped .cfg's binding, accepted / refused for a corpus of .cfg
texts (the rejection tests' own, and the cases the two front ends used to read differently), and the text of about twenty
reachable states per model family.  (tests/test_cfg_cli_cpu.py sends every refused text through both executables.)"""
import json
import os

import pytest

from kafka_specification_amd import CheckerConfig
from kafka_specification_amd.cfg import CfgError, parse_cfg, to_checker_config
from kafka_specification_amd.format import format_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "frontend_parity.json")))
REFUSED = [r for r in GOLDEN["refusals"] if not r["accepted"]]
CONSTANTS = ("n_replicas", "log_size", "max_records", "max_leader_epoch", "n_log_records", "max_id")


def test_every_shipped_cfg_binds_as_recorded():
    shipped = sorted(f for f in os.listdir(os.path.join(ROOT, "models")) if f.endswith(".cfg"))
    assert shipped == sorted(GOLDEN["bindings"]) and len(shipped) == 14
    for name, want in GOLDEN["bindings"].items():
        c = to_checker_config(want["module"], parse_cfg(open(os.path.join(ROOT, "models", name)).read()))
        got = dict(module=want["module"], model=c.model, **{k: getattr(c, k) for k in CONSTANTS},
                   invariants=list(c.invariants), check_deadlock=c.check_deadlock)
        assert got == want, name


def test_the_corpus_is_accepted_and_refused_as_recorded():
    assert len(GOLDEN["refusals"]) == 44 and len(REFUSED) == 36
    for r in GOLDEN["refusals"]:
        try:
            to_checker_config(r["module"], parse_cfg(r["text"]))
            accepted = True
        except CfgError:
            accepted = False
        assert accepted == r["accepted"], (r["module"], r["text"])


def test_states_print_as_recorded():
    assert sorted(s["config"]["model"] for s in GOLDEN["states"]) == ["AsyncIsr", "FiniteReplicatedLog", "IdSequence", "Kip279", "Kip320"]
    for s in GOLDEN["states"]:
        cfg = CheckerConfig(**s["config"])
        assert len(s["cases"]) >= 16
        for canon, text in s["cases"]:
            assert format_state(cfg, bytes.fromhex(canon)) == text, (s["config"], canon)
        with pytest.raises(ValueError):                       # a state shorter than the constants' layout is refused, not read
            format_state(cfg, bytes.fromhex(s["cases"][0][0])[:-1])
