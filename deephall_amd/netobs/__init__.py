"""NetObs bridge (deephall/netobs_bridge/*) on the native kernels.

The reference plugs DeepHall into the third-party NetObs framework (``netobs``, absent
here): an adaptor that restores a checkpoint and exposes the network, the MCMC walk and the
energies (adaptor.py:36-115), a ``HallSystem`` (hall_system.py), and four estimators
(observables/density.py, pair_corr.py, overlap.py, one_rdm.py).  This package mirrors them
with the same names, options, value/state keys and digests:

* histograms (density, pair correlation) and the lowest-Landau-level monopole harmonics of
  the one-body density matrix are HIP kernels (csrc/netobs.hip, ``dh_histograms``,
  ``dh_monopole_orbitals``);
* the Renyi-2 entanglement entropy of a polar cap (observables/renyi2.py, not in the reference)
  classifies, compacts and reduces its swapped walker pairs in csrc/swap.hip (``dh_swap_*``);
  ``entanglement.filled_lll_cap`` is the exact filled-Landau-level answer to check it against;
* the one-body density matrix resolved by Landau level (observables/ll_rdm.py, not in the
  reference): the basis Y_{Q,Q+n,m} of the first few levels, the displaced rows and the reduction
  over walkers and r' points in double are csrc/rdm.hip (``dh_monopole_harmonics``, ``dh_rdm_*``);
  its digest gives the occupation of each level and the weight above the last one kept;
* the total spin <S^2> (observables/spin_square.py, not in the reference) exchanges one up and one
  down electron: the exchanged rows, the ratios and the reduction over walkers in double are
  csrc/spin.hip (``dh_spin_*``); S (S + 1) on every walker of a total-spin eigenstate;
* the static structure factor S(L) with its partial, spin, connected and guiding-centre forms
  (observables/structure_factor.py, not in the reference) needs the walkers only: the Legendre pair
  sums, the multipoles sum_i Y_LM and their reduction over walkers in double are csrc/sfactor.hip
  (``dh_sf_*``);
* the overlap matrix of a pinned-quasihole state with its holes moved (observables/hole_overlap.py,
  not in the reference): log psi of K hole configurations on the same walkers in double and the
  K x K Gram matrix of their ratios are csrc/quasihole.hip and csrc/holes.hip (``dh_hole_*``);
  holonomy.py turns the overlaps into Berry phases and non-Abelian holonomies on the host;
* the density around any axis and the excess charge inside a cap about it
  (observables/axis_density.py, not in the reference): equal-area bins of r_i . a, integer counts by
  species in csrc/impurity.hip (``dh_axis_histogram``); the axis can be one of ``system.impurities``,
  whose potential the adaptor's potential energy includes (``dh_external_potential``);
* the pair amplitudes A_L, the mean number of pairs with pair angular momentum L in the lowest Landau
  level (observables/pair_amplitude.py, not in the reference): the rows with two electrons displaced
  and the reduction of the ratios times the pair projector over walkers, points and pairs in double
  are csrc/pairamp.hip (``dh_pair_*``); pseudopotential.py turns A_L into the energy of any pair
  interaction through its Haldane pseudopotentials on the host;
* the energies in the span of K wavefunctions (observables/subspace.py, not in the reference): the
  run's own network and up to 31 trial states on its walkers, one ``dh_local_energy`` call per state,
  and the K x K overlap, Hamiltonian and kinetic matrices of their ratios and local energies summed
  in double in csrc/subspace.hip (``dh_subspace_accumulate``); subspace.py Hermitises them, drops the
  linearly dependent directions and solves H v = E S v on the host: an excitation spectrum (CF
  excitons of each L from their determinants), and the same at another interaction strength;
* every wavefunction value goes through ``dh_logpsi`` (Psiformer or the native Laughlin
  state), the walk through ``dh_mcmc_step``;
* ``evaluate`` is a minimal stand-in for NetObs's own evaluation loop (restore, burn-in,
  walk + evaluate per step, digest), which cannot be pinned here (the package is absent):
  per step it stores the walker mean of each value, as the estimators' ``empty_val_state``
  shapes (steps, *observable shape) imply.
"""

from .adaptor import DeepHallAdaptor, DeepHallAuxData
from .estimator import Estimator, Observable, evaluate
from .hall_system import HallSystem
from . import subspace  # the host solver (netobs.subspace); the estimator is observables.subspace
from .observables import (axis_density, density, hole_overlap, ll_rdm, one_rdm, overlap, pair_amplitude, pair_corr,
                          renyi2, spin_square, structure_factor)
from .observables import subspace as subspace_estimator


class _Registry(dict):
    """Estimators by name.  The dict's own keys — what iterating, ``len`` and ``in`` see — are a
    pinned list; ``registry[name]`` and ``.get(name)`` also find the names of ``more``."""

    def __init__(self, own, more):
        super().__init__(own)
        self.more = more

    def __missing__(self, name):
        return self.more[name]

    def get(self, name, default=None):
        try:
            return self[name]
        except KeyError:
            return default


# Estimators the reference does not have (no ``deephall@`` name in cli_extend.py).  The listed key
# is the first of them, which tests/test_renyi2_host.py pins as the whole set; the later ones are
# looked up by name, EXTRA_ESTIMATORS["ll_rdm"], and listed in EXTRA_ESTIMATORS.more.
EXTRA_ESTIMATORS = _Registry({
    "renyi2": renyi2.DEFAULT,
}, more={
    "ll_rdm": ll_rdm.DEFAULT,
    "spin_square": spin_square.DEFAULT,
    "structure_factor": structure_factor.DEFAULT,
    "hole_overlap": hole_overlap.DEFAULT,
    "axis_density": axis_density.DEFAULT,
    "pair_amplitude": pair_amplitude.DEFAULT,
    "subspace": subspace_estimator.DEFAULT,
})

# The own keys are the reference's ``deephall@`` names, so the registry still lists exactly what
# cli_extend.py registers; ESTIMATORS[name] also finds EXTRA_ESTIMATORS.
ESTIMATORS = _Registry({
    "density": density.DEFAULT,
    "pair_corr": pair_corr.DEFAULT,
    "overlap": overlap.DEFAULT,
    "one_rdm": one_rdm.DEFAULT,
}, more=EXTRA_ESTIMATORS)

__all__ = ["DeepHallAdaptor", "DeepHallAuxData", "Estimator", "Observable", "HallSystem", "evaluate", "ESTIMATORS",
           "EXTRA_ESTIMATORS"]
