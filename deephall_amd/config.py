"""Configuration dataclasses — the fields of deephall/config.py:56-214 the hot path reads.

Field names, defaults and meaning follow the reference exactly (System 56-79,
PsiformerNetwork 92-97, Network 100-104, MCMC 107-122, LearningRate / optimizers
125-165, Log 168-198, Config 201-214).  The
OmegaConf machinery is out of scope; ``Config.from_dict`` mirrors the reference's
``from_dict`` (config.py:23-48: nested dataclasses, extra keys ignored).
The reference needs Python >= 3.11 (``StrEnum``); these are ``str`` Enums.
"""

from __future__ import annotations

import enum
import time
from dataclasses import dataclass, field, fields, is_dataclass
from typing import Any, Optional, Tuple


def from_dict(cls, dikt: dict):
    try:
        ftypes = {f.name: f.type for f in fields(cls)}
        resolved = {f.name: f for f in fields(cls)}
        kwargs = {}
        for k, v in dikt.items():
            if k not in ftypes:
                continue  # allow extra keys (config.py:41)
            default = resolved[k].default_factory() if callable(resolved[k].default_factory) else None
            if is_dataclass(default) and isinstance(v, dict):
                kwargs[k] = from_dict(type(default), v)
            else:
                kwargs[k] = v
        return cls(**kwargs)
    except Exception as e:  # noqa: BLE001
        raise ValueError(f"Error converting dictionary to {cls.__name__}: {e}") from e


class InteractionType(str, enum.Enum):
    coulomb = "coulomb"
    harmonic = "harmonic"


class NetworkType(str, enum.Enum):
    psiformer = "psiformer"
    laughlin = "laughlin"
    jain = "jain"
    pfaffian = "pfaffian"
    halperin = "halperin"
    quasihole = "quasihole"


class OrbitalType(str, enum.Enum):
    full = "full"
    sparse = "sparse"


IMPURITY_KINDS = ("gaussian", "charge")
IMPURITY_SPECIES = ("both", "up", "down")
MAX_IMPURITIES = 8


@dataclass(frozen=True)
class Impurity:
    """A local one-body potential pinned at (theta, phi) (not in the reference; csrc/impurity.hip).
    With R the sphere's radius and c^2 = 2 R^2 (1 - cos gamma) the squared chord to an electron,
    ``kind`` "gaussian": strength exp(-c^2 / (2 width^2)); "charge": strength / sqrt(c^2 + width^2),
    a point charge at the height ``width`` above the surface.  ``width`` is in magnetic lengths, the
    unit of ``System.radius``, and > 0.  ``strength`` > 0 repels the electrons (pins a quasihole).
    ``species``: "both", "up" or "down", the words of ``network.quasihole.species``."""

    theta: float
    phi: float
    strength: float
    kind: str = "gaussian"
    width: float = 1.0
    species: str = "both"

    def __post_init__(self):
        for name in ("theta", "phi", "strength", "width"):
            object.__setattr__(self, name, float(getattr(self, name)))
        for name in ("kind", "species"):
            v = getattr(self, name)
            object.__setattr__(self, name, str(getattr(v, "value", v)))
        if self.kind not in IMPURITY_KINDS:
            raise ValueError(f"impurity: kind {self.kind!r} is not one of {IMPURITY_KINDS}")
        if self.species not in IMPURITY_SPECIES:
            raise ValueError(f"impurity: species {self.species!r} is not one of {IMPURITY_SPECIES}")
        if not self.width > 0.0:
            raise ValueError(f"impurity: width must be > 0, got {self.width}")


def as_impurities(entries) -> tuple:
    """A tuple of `Impurity` from Impurity objects, dicts of its fields or sequences in field order
    (theta, phi, strength[, kind, width, species]): what a config file can hold."""
    out = []
    for e in entries or ():
        if isinstance(e, Impurity):
            out.append(e)
        elif isinstance(e, dict):
            out.append(Impurity(**e))
        else:
            out.append(Impurity(*e))
    if len(out) > MAX_IMPURITIES:
        raise ValueError(f"impurity: at most {MAX_IMPURITIES} impurities, got {len(out)}")
    return tuple(out)


@dataclass
class System:
    flux: int = 2
    radius: Optional[float] = None
    nspins: Tuple[int, int] = (3, 0)
    interaction_strength: float = 1.0
    lz_center: float = 0.0
    lz_penalty: float = 0.0
    l2_penalty: float = 0.0
    interaction_type: InteractionType = InteractionType.coulomb
    impurities: tuple = ()  # of Impurity; not in the reference

    def __post_init__(self):
        self.impurities = as_impurities(self.impurities)  # lists or dicts from a config file


@dataclass
class PsiformerNetwork:
    num_heads: int = 4
    heads_dim: int = 64
    num_layers: int = 2
    determinants: int = 1


@dataclass
class JainNetwork:
    """Jain composite-fermion state with two Lambda levels (not in the reference; networks/jain.py).
    ``cf_flux``: p, 2p vortices per electron.  ``occupation``: N pairs (n, m), Lambda level n in
    {0, 1} and |m| <= Q1 + n, one determinant column each; None is the ground state with both
    levels filled (N = 4 Q1 + 4)."""

    cf_flux: int = 1
    occupation: Optional[tuple] = None

    def __post_init__(self):
        if self.occupation is not None:  # a list of [n, m] lists from a config file
            self.occupation = tuple((int(n), float(m)) for n, m in self.occupation)


@dataclass
class PfaffianNetwork:
    """Moore-Read Pfaffian state (not in the reference; networks/pfaffian.py).  ``cf_flux``: p,
    2p vortices per electron; the system's flux must be 2p (N - 1) - 1 with N even."""

    cf_flux: int = 1


@dataclass
class HalperinNetwork:
    """Halperin (m_up, m_dn, n) two-component state (not in the reference; networks/halperin.py).
    ``exponents``: (m_up, m_dn, n), the intra-species exponents odd, n >= 0; the system's flux must
    be m_up (n_up - 1) + n n_dn and m_dn (n_dn - 1) + n n_up.  The default is the singlet at 2/5."""

    exponents: tuple = (3, 3, 2)

    def __post_init__(self):
        self.exponents = tuple(int(e) for e in self.exponents)  # a list from a config file


@dataclass
class QuasiholeNetwork:
    """Quasiholes pinned at chosen points (not in the reference; networks/quasihole.py).  ``base``:
    "halperin" (exponents from ``network.halperin.exponents``; Laughlin 1/m is nspins (N, 0)) or
    "pfaffian" (p from ``network.pfaffian.cf_flux``).  ``holes``: (theta, phi) pairs, at most 8.
    ``species``: "both", "up" or "down" per hole, halperin base only; None is all "both".
    ``pairing``: two equal-length tuples of hole indices, the groups A and B of the pfaffian base;
    the holes not listed are Abelian.  The system's flux rises by one per hole that acts on a
    species (halperin base), by one per pair of the groups and per Abelian hole (pfaffian base)."""

    base: str = "halperin"
    holes: tuple = ()
    species: Optional[tuple] = None
    pairing: Optional[tuple] = None

    def __post_init__(self):  # lists from a config file
        self.base = str(getattr(self.base, "value", self.base))
        self.holes = tuple((float(t), float(p)) for t, p in self.holes)
        if self.species is not None:
            self.species = tuple(str(s) for s in self.species)
        if self.pairing is not None:
            self.pairing = tuple(tuple(int(a) for a in grp) for grp in self.pairing)


@dataclass
class Network:
    type: NetworkType = NetworkType.psiformer
    orbital: OrbitalType = OrbitalType.full
    psiformer: PsiformerNetwork = field(default_factory=PsiformerNetwork)
    jain: JainNetwork = field(default_factory=JainNetwork)
    pfaffian: PfaffianNetwork = field(default_factory=PfaffianNetwork)
    halperin: HalperinNetwork = field(default_factory=HalperinNetwork)
    quasihole: QuasiholeNetwork = field(default_factory=QuasiholeNetwork)


@dataclass
class MCMC:
    steps: int = 10
    width: float = 0.1
    burn_in: int = 200
    adapt_frequency: int = 100


@dataclass
class LearningRate:
    """rate * (1 / (1 + t / delay)) ** decay (config.py:125-137)."""

    rate: float = 0.005
    decay: float = 1.0
    delay: float = 2000.0

    def schedule(self, t):
        return self.rate * (1.0 / (1.0 + (t / self.delay))) ** self.decay


class OptimizerName(str, enum.Enum):
    adam = "adam"
    kfac = "kfac"
    minsr = "minsr"
    none = "none"


@dataclass
class OptimizerAdam:
    lr: LearningRate = field(default_factory=LearningRate)


@dataclass
class OptimizerKfac:
    lr: LearningRate = field(default_factory=lambda: LearningRate(rate=0.05))


@dataclass
class OptimizerMinsr:
    """MinSR (optimizers.py make_minsr_training_step; not in the reference): the three knobs play
    the roles of KFAC's here (optimizers.py KFAC_DAMPING, KFAC_NORM_CONSTRAINT) and start from
    its values.  ``sharded``: the Gram matrix is computed in shares across the ranks
    (optimizers.minsr_direction_sharded); opt-in, because every rank then holds the gathered
    batch's activations and the (2 x global batch)^2 matrices.  Without it MinSR runs on one rank
    only.  ``momentum``: SPRING's mu (Goldshlager, Abrahamsen, Lin 2024), 0 <= mu < 1; the
    damping then pulls the step towards mu x the previous one instead of towards 0.  0: MinSR."""

    lr: LearningRate = field(default_factory=lambda: LearningRate(rate=0.05))
    damping: float = 1e-3
    norm_constraint: float = 1e-3
    sharded: bool = False
    momentum: float = 0.0


@dataclass
class Pretrain:
    """Fidelity pretraining onto a trial state before the energy minimisation (pretrain.py; not
    in the reference).  ``iterations``: 0 switches it off.  ``reference``: "laughlin", "jain",
    "pfaffian", "halperin" or "quasihole", built for the run's system as the overlap estimator builds it
    (``network.jain`` / ``network.pfaffian`` choose p and the occupation, ``network.halperin`` the
    exponents, ``network.quasihole`` the base and the holes).  ``lr``: None is the chosen optimizer's own
    schedule; either way it starts at t = 0 and the training after it starts at t = 0 again."""

    iterations: int = 0
    reference: str = "laughlin"
    lr: Optional[LearningRate] = None

    def __post_init__(self):
        if isinstance(self.lr, dict):  # from a config file
            self.lr = from_dict(LearningRate, self.lr)


@dataclass
class Orthogonal:
    """Overlap penalties against frozen lower states, for excited states (orthogonal.py; not in the
    reference): the energy phase minimises E + sum_k lambda_k F_k.  ``states``: () switches it off.
    An entry is a trial state in the ``subspace`` estimator's form, ``{type: laughlin | jain |
    pfaffian | halperin | quasihole, <sub-configs>}``, or a Psiformer checkpoint ``{checkpoint: <file
    or directory>, psiformer: {...}?, orbital: ...?}``; either takes an optional ``penalty`` >= 0,
    its lambda_k.  ``penalty``: lambda_k of the entries that name none; it should exceed the gap to
    the state.  At most 16 states."""

    states: tuple = ()
    penalty: float = 1.0

    def __post_init__(self):  # a list of dicts from a config file
        self.states = tuple(dict(s) if isinstance(s, dict) else s for s in (self.states or ()))


@dataclass
class Optim:
    """config.py:160-165.  The default optimizer is KFAC, as in the reference
    (optimizers.py: make_kfac_training_step on the dh_kfac_* kernels)."""

    iterations: int = 1000
    optimizer: Optional[OptimizerName] = OptimizerName.kfac
    adam: OptimizerAdam = field(default_factory=OptimizerAdam)
    kfac: OptimizerKfac = field(default_factory=OptimizerKfac)
    minsr: OptimizerMinsr = field(default_factory=OptimizerMinsr)
    pretrain: Pretrain = field(default_factory=Pretrain)
    orthogonal: Orthogonal = field(default_factory=Orthogonal)


@dataclass
class Log:
    """config.py:168-198."""

    save_path: Optional[str] = None
    restore_path: Optional[str] = None
    save_time_interval: int = 10 * 60
    save_step_interval: int = 1000
    initial_energy: bool = True


@dataclass
class Config:
    batch_size: int = 3360
    seed: int = field(default_factory=lambda: int(time.time()))
    system: System = field(default_factory=System)
    network: Network = field(default_factory=Network)
    mcmc: MCMC = field(default_factory=MCMC)
    optim: Optim = field(default_factory=Optim)
    log: Log = field(default_factory=Log)

    @classmethod
    def from_dict(cls, dikt: dict[str, Any]) -> "Config":
        return from_dict(cls, dikt)
