#!/usr/bin/env python3
"""What the .cfg reader binds, what it refuses and how a state prints — recorded from the Python front end (cfg.py, format.py)
as it stood BEFORE both front ends were moved onto csrc/kmc_frontend.cpp, so that the library's answers can be held against
the implementation it replaced (tests/test_frontend_parity_cpu.py).  Run today it goes through the library and must
reproduce the committed file byte for byte.

    python tests/golden/make_frontend_parity.py        # writes tests/golden/frontend_parity.json
"""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# root module of the shipped .cfg files whose name is not the module's (tests/test_cfg_cli_cpu.py)
MODULE_OF = {"Kip279_5brokers": "Kip279", "Kip320_7brokers": "Kip320", "LeaderInIsr": "Kip320",
             "KafkaTruncateToHighWatermark_3brokers": "KafkaTruncateToHighWatermark",
             "MCAsyncIsr_small": "MCAsyncIsr", "MCAsyncIsr_outside": "MCAsyncIsr"}
CONSTANTS = ("n_replicas", "log_size", "max_records", "max_leader_epoch", "n_log_records", "max_id")


def corpus():
    """(module, .cfg text): the rejections of test_cfg_cli_cpu.py and test_async_isr_cpu.py, the cases on which the two front
    ends used to disagree, and a few accepted neighbours of each."""
    asy = open(os.path.join(ROOT, "models", "MCAsyncIsr_small.cfg")).read()
    kip = open(os.path.join(ROOT, "models", "Kip320.cfg")).read()
    frl = "CONSTANTS Replicas = {a, b}\n LogRecords = {x}\n Nil = %s\n LogSize = 3\nCHECK_DEADLOCK FALSE"
    return [
        # tests/test_cfg_cli_cpu.py::test_cfg_rejections
        ("IdSequence", "SYMMETRY Perms\nCONSTANT MaxId = 1"),
        ("Kip320", "CONSTANTS Replicas = {b1, NONE}\nLogSize=1\nMaxRecords=1\nMaxLeaderEpoch=1"),
        ("Kip320", "CONSTANTS Replicas = {b1, b2}\nLogSize=1\nMaxRecords=1"),
        ("IdSequence", "CONSTANT MaxId = 1\nINVARIANT StrongIsr"),
        ("AsyncIsr", "CONSTANT MaxId = 1"),
        ("KafkaReplication", "CONSTANT MaxId = 1"),
        ("IdSequence", "CONSTANT MaxId = 1\nPROPERTY Live"),
        ("IdSequence", "CONSTANT MaxId <- SmallId"),
        ("IdSequence", "CONSTANT MaxId = many"),
        ("Kip320", "CONSTANTS Replicas = {b1, b2}\nLogSize=two\nMaxRecords=1\nMaxLeaderEpoch=1"),
        ("IdSequence", "CONSTANT MaxId = 1\nSPECIFICATION Spec\nINIT Init\nNEXT Next"),
        # tests/test_async_isr_cpu.py::test_cfg_rejects_what_it_cannot_honour
        ("AsyncIsr", asy),
        ("MCAsyncIsr", asy.replace("CONSTRAINT StateConstraint", "")),
        ("MCAsyncIsr", asy.replace("StateConstraint", "SomethingElse")),
        ("MCAsyncIsr", asy.replace("Leader = r1", "Leader = r9")),
        ("MCAsyncIsr", asy.replace("ValidHighWatermark", "StrongIsr")),
        ("Kip320", kip + "\nCONSTRAINT StateConstraint\n"),
        # where the native reader used to be the laxer one
        ("IdSequence", "CONSTANT MaxId = 1\nCHECK_DEADLOCK MAYBE"),
        ("MCAsyncIsr", asy.replace("{r1, r2, r3}", "{r1, r2, r2}")),
        ("Kip320", kip.replace("{b1, b2, b3}", "{b1, b2, b1}")),
        ("MCAsyncIsr", asy.replace("MaxOffset = 3", "MaxOffset = 0")),
        ("MCAsyncIsr", asy.replace("{r1, r2, r3}", "{r10, r2}")),
        ("Kip320", kip.replace("{b1, b2, b3}", '{b1, "NONE"}')),
        ("Kip320", kip.replace("{b1, b2, b3}", "{b1, NONE2}")),
        ("FiniteReplicatedLog", frl % '"a b"'),
        ("MCAsyncIsr", asy.replace("Leader = r1", 'Leader = "r1"')),
        ("IdSequence", "CONSTANT MaxId ="),
        ("IdSequence", "CONSTANT MaxId = 1\nINVARIANT TypeOk\nCONSTANT X ="),
        # accepted neighbours (tests/test_cfg_cli_cpu.py::test_cfg_syntax) and the other refusals of the reader
        ("IdSequence", "\n (* block\n    comment *)\n CONSTANT MaxId = 7   \\* trailing comment\n SPECIFICATION Spec\n INVARIANT TypeOk\n"),
        ("IdSequence", "CONSTANT MaxId = 7\nSPECIFICATION Other"),
        ("IdSequence", "CONSTANT MaxId = 7\nINIT Start"),
        ("IdSequence", "CONSTANT MaxId = 7\nNEXT Step"),
        ("FiniteReplicatedLog", frl % "nil"),
        ("FiniteReplicatedLog", (frl % "nil").replace("{a, b}", "a")),
        ("FiniteReplicatedLog", (frl % "nil").replace(" Nil = nil\n", "")),
        ("IdSequence", "MaxId = 7"),
        ("IdSequence", "CONSTANT MaxId 7"),
        ("IdSequence", "CONSTANT MaxId = TRUE"),
        ("IdSequence", "CONSTANT MaxId = -3\nCHECK_DEADLOCK TRUE"),
        ("IdSequence", "CONSTANT MaxId=7 INVARIANT TypeOk TypeOk"),
        ("Kip320", kip.replace("{b1, b2, b3}", "{}")),
        ("Kip320", kip.replace("LogSize = 6", "LogSize = {6}")),
        ("Kip320", kip.replace("INVARIANTS", "VIEW v\nINVARIANTS")),
        ("Kip320", kip.replace("CONSTANTS", "ACTION_CONSTRAINT a\nCONSTANTS")),
    ]


def special(model, b, N, L):
    """A state worth printing whatever the sample holds: an empty ISR, a "NONE" leader, a full log."""
    if model == "AsyncIsr":
        return b[0] == 0 or b[2] == 0 or b[4] == 0 or b[6] == L
    if model == "FiniteReplicatedLog":
        return any(b[r * (1 + L)] == L for r in range(N))
    if model == "IdSequence":
        return False
    rs = 5 + L
    return any(b[r * rs] == L or b[r * rs + 4] == 0 or b[r * rs + 3] == 0 for r in range(N)) or b[N * rs + 3] == 0


def main():
    import kmo
    from kafka_specification_amd import CheckerConfig
    from kafka_specification_amd.cfg import CfgError, parse_cfg, to_checker_config
    from kafka_specification_amd.format import format_state

    bindings = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "models", "*.cfg"))):
        name = os.path.splitext(os.path.basename(path))[0]
        module = MODULE_OF.get(name, name)
        c = to_checker_config(module, parse_cfg(open(path).read()))
        bindings[name + ".cfg"] = dict(module=module, model=c.model, **{k: getattr(c, k) for k in CONSTANTS},
                                       invariants=list(c.invariants), check_deadlock=c.check_deadlock)

    refusals = []
    for module, text in corpus():
        try:
            to_checker_config(module, parse_cfg(text))
            accepted = True
        except CfgError:
            accepted = False
        refusals.append(dict(module=module, text=text, accepted=accepted))

    states = []
    for model, N, L, R, E, K, max_id in [("Kip320", 2, 2, 2, 1, 2, 10), ("Kip279", 3, 2, 2, 2, 2, 10),
                                         ("FiniteReplicatedLog", 2, 3, 2, 1, 1, 10), ("IdSequence", 3, 2, 2, 1, 2, 24),
                                         ("AsyncIsr", 3, 3, 2, 4, 2, 10)]:
        o = kmo.Run(kmo.make_config(model, N=N, L=L, R=R, E=E, K=K, MaxId=max_id, invariants=(), max_states=3000, threads=1))
        n = min(o.distinct, 3000)
        picked = list(range(0, n, max(1, n // 16)))[:16]          # the initial state is index 0
        spec = [i for i in range(n) if special(model, o.state(i), N, L)]
        for i in ([spec[0], spec[len(spec) // 3], spec[2 * len(spec) // 3], spec[-1]] if spec else []):
            if i not in picked:
                picked.append(i)
        cc = CheckerConfig(model=model, n_replicas=N, log_size=L, max_records=R, max_leader_epoch=E, n_log_records=K, max_id=max_id)
        states.append(dict(config=dict(model=model, **{k: getattr(cc, k) for k in CONSTANTS}),
                           cases=[[o.state(i).hex(), format_state(cc, o.state(i))] for i in picked]))
        o.close()

    out = os.path.join(ROOT, "tests", "golden", "frontend_parity.json")
    with open(out, "w") as f:
        json.dump(dict(bindings=bindings, refusals=refusals, states=states), f, indent=1, sort_keys=True)
        f.write("\n")
    print(out, os.path.getsize(out), "bytes;", sum(len(s["cases"]) for s in states), "states,", len(refusals), "cfg texts,",
          sum(1 for r in refusals if not r["accepted"]), "refused")


if __name__ == "__main__":
    main()
