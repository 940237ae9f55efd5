"""kmc_successors_batch without a GPU: what it refuses, and its code object's place in the cache."""
import os

import numpy as np
import pytest

from kafka_specification_amd import CheckerConfig, KmcError, ModelChecker, compiler_identity, precompile, precompile_batch

SMALL = dict(model="Kip101", n_replicas=2, log_size=3, max_records=2, max_leader_epoch=1)


@pytest.mark.parametrize("kw,spl,code", [
    (dict(model="Kip320"), 0, 5),                             # KMC_E_STATE: a host-only handle
    (dict(model="Kip320"), (1 << 22) + 1, 1),                  # KMC_E_ARG: states_per_launch beyond 2^22
    (dict(model="Kip320", symmetry=True), 0, 1),               # ... a handle that counts orbits
    (dict(model="AsyncIsr", n_replicas=2, log_size=2, max_leader_epoch=2), 0, 1),   # ... AsyncIsr
])
def test_what_a_batch_refuses(kw, spl, code):
    with ModelChecker(CheckerConfig(device=-1, **kw)) as mc:
        states = np.zeros((3, mc.state_words), dtype=np.uint64)
        with pytest.raises(KmcError) as e:
            mc.successors_batch(states, states_per_launch=spl)
        assert e.value.code == code and str(e.value).split(": ", 1)[1]   # the reason is in kmc_last_error


def test_the_batch_object_has_a_file_of_its_own(tmp_path):
    cfg = CheckerConfig(cache_dir=str(tmp_path), **SMALL)
    precompile_batch(cfg, "gfx950")
    files = os.listdir(tmp_path / "batch")
    assert os.listdir(tmp_path) == ["batch"] and len(files) == 1
    assert files[0].startswith("Kip101_N2_L3_R2_E1-gfx950-") and files[0].endswith(f"-c{compiler_identity(0)}-batch.hsaco")
    assert open(tmp_path / "batch" / files[0], "rb").read(4) == b"\x7fELF"
    precompile(cfg, "gfx950")   # the search's three objects stay three
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]) == 3 and len(os.listdir(tmp_path / "batch")) == 1
    for refused in (dict(symmetry=True), dict(model="AsyncIsr")):
        with pytest.raises(KmcError):
            precompile_batch(CheckerConfig(cache_dir=str(tmp_path), **{**SMALL, **refused}), "gfx950")
