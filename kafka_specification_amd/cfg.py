"""TLC's model-configuration (.cfg) syntax, as far as these specs need it [TLC-recall]: the reader and its binding to the
lowered models live in the library (csrc/kmc_frontend.cpp: kmc_cfg_bind), where the native command line finds them too;
this is its ctypes face.  What is read and what is refused, with the reasons: include/kmc.h, "front end"."""
from __future__ import annotations

import ctypes as C

from . import _native as nat
from .checker import CheckerConfig

# root modules whose lowered model carries another name: the MC module adds the state constraint
MODULE_TO_MODEL = {"MCAsyncIsr": "AsyncIsr"}


class CfgError(ValueError):
    pass


class ModelCfg(str):
    """The text of a .cfg: it is read when it is bound to a module (to_checker_config)."""


def parse_cfg(text: str) -> ModelCfg:
    return ModelCfg(text)


def to_checker_config(module: str, cfg: str, **overrides) -> CheckerConfig:
    """Bind a .cfg to the lowered model of `module` (the root module's name); CfgError for what cannot be honoured."""
    c = CheckerConfig(model="IdSequence", invariants=()).to_native()      # constants the .cfg does not bind keep their defaults
    if nat.lib().kmc_cfg_bind(module.encode(), cfg.encode(), C.byref(c)) != 0:
        raise CfgError(nat.lib().kmc_last_error().decode("utf-8", "replace"))
    model = nat.lib().kmc_model_name(c.model).decode()
    kw = dict(model=model, n_replicas=c.n_replicas, log_size=c.log_size, max_records=c.max_records,
              max_leader_epoch=c.max_leader_epoch, n_log_records=c.n_log_records, max_id=c.max_id,
              invariants=tuple(n for n, bit in nat.invariant_bits(model).items() if c.invariant_mask & bit),
              check_deadlock=bool(c.check_deadlock))
    kw.update(overrides)
    return CheckerConfig(**kw)
