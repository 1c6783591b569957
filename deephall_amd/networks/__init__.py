"""make_network (deephall/networks/__init__.py:22-37)."""

from __future__ import annotations

from ..config import Network, NetworkType, System
from .halperin import Halperin, HalperinCallable
from .jain import Jain, JainCallable
from .laughlin import Laughlin, LaughlinQuasiparticle
from .pfaffian import MooreRead, MooreReadCallable
from .psiformer import Psiformer
from .quasihole import Quasihole, QuasiholeCallable


def make_network(system: System, network: Network) -> Psiformer:
    Q = system.flux / 2
    ntype = str(getattr(network.type, "value", network.type))
    if ntype == NetworkType.laughlin.value:  # networks/__init__.py:24-27 (ground state, quasihole and
        # quasiparticle fillings all run on laughlin.hip)
        return Laughlin(flux=system.flux, nspins=system.nspins, excitation_lz=system.lz_center, system=system)
    if ntype == NetworkType.jain.value:  # cf.hip; occupation None: both Lambda levels filled
        return Jain(flux=system.flux, nspins=system.nspins, cf_flux=network.jain.cf_flux,
                    occupation=network.jain.occupation, system=system)
    if ntype == NetworkType.pfaffian.value:  # pfaffian.hip: Moore-Read at flux 2p(N-1)-1
        return MooreRead(flux=system.flux, nspins=system.nspins, cf_flux=network.pfaffian.cf_flux, system=system)
    if ntype == NetworkType.halperin.value:  # halperin.hip: (m_up, m_dn, n) on the two species of nspins
        return Halperin(flux=system.flux, nspins=system.nspins, exponents=network.halperin.exponents, system=system)
    if ntype == NetworkType.quasihole.value:  # quasihole.hip: pinned holes on the halperin or the pfaffian base
        q = network.quasihole
        return Quasihole(flux=system.flux, nspins=system.nspins, base=q.base, holes=q.holes, species=q.species,
                         pairing=q.pairing, exponents=network.halperin.exponents, cf_flux=network.pfaffian.cf_flux,
                         system=system)
    if ntype == NetworkType.psiformer.value:
        return Psiformer(
            Q=Q,
            nspins=system.nspins,
            ndets=network.psiformer.determinants,
            num_heads=network.psiformer.num_heads,
            num_layers=network.psiformer.num_layers,
            heads_dim=network.psiformer.heads_dim,
            orbital_type=network.orbital,
            system=system,
        )
    raise ValueError(f"unknown network type {network.type}")


__all__ = ["make_network", "Psiformer", "Laughlin", "LaughlinQuasiparticle", "Jain", "JainCallable",
           "MooreRead", "MooreReadCallable", "Halperin", "HalperinCallable",
           "Quasihole", "QuasiholeCallable"]
