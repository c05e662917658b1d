"""
:class:`GNM` — Gaussian Network Model (host mirror of the reference's gnm.py:20-303).
"""

from . import nma
from ._model import ElasticNetworkModel

__all__ = ["GNM"]

K_B = nma.K_B
N_A = nma.N_A


class GNM(ElasticNetworkModel):
    """
    Gaussian Network Model.

    Parameters
    ----------
    atoms : AtomArray, shape=(n,) or ndarray, shape=(n,3), dtype=float
    force_field : ForceField, natoms=n
    masses : bool or ndarray, shape=(n,), dtype=float, optional
    use_cell_list : bool, optional
        Interface compatibility only.

    Attributes
    ----------
    kirchhoff : ndarray, shape=(n,n), dtype=float.  Not a copy.
    covariance : ndarray, shape=(n,n), dtype=float  (pseudo-inverse of the Kirchhoff matrix).  Not a copy.
    masses : None or ndarray, shape=(n,), dtype=float
    """

    _dim = 1

    @property
    def kirchhoff(self):
        return self._get_matrix()

    @kirchhoff.setter
    def kirchhoff(self, value):
        # the reference raises ValueError here and IndexError in every other setter (gnm.py:115-120)
        self._set_matrix(value, ValueError)

    @property
    def covariance(self):
        return self._get_covariance()

    @covariance.setter
    def covariance(self, value):
        self._set_covariance(value)

    def eigen(self, subset_by_index=None, subset_by_value=None):
        """
        Eigenvalues (ascending, (n,)) and eigenvectors (rows, (n,n)) of the Kirchhoff matrix (gnm.py:145-158).
        ``subset_by_index`` / ``subset_by_value``: a part of the spectrum only, see :func:`nma.eigen`.
        """
        return nma.eigen(self, subset_by_index, subset_by_value)

    def frequencies(self):
        """Mode frequencies in arbitrary units (gnm.py:160-176)."""
        return nma.frequencies(self)

    def mean_square_fluctuation(self, mode_subset=None, tem=None, tem_factors=K_B):
        """Per-atom mean square fluctuation (gnm.py:178-212)."""
        return nma.mean_square_fluctuation(self, mode_subset, tem, tem_factors)

    def bfactor(self, mode_subset=None, tem=None, tem_factors=K_B):
        """Isotropic B-factors (gnm.py:214-244)."""
        return nma.bfactor(self, mode_subset, tem, tem_factors)

    def dcc(self, mode_subset=None, norm=True, tem=None, tem_factors=K_B):
        """Dynamic cross-correlation (n,n) (gnm.py:246-303)."""
        return nma.dcc(self, mode_subset, norm, tem, tem_factors)

    def correlation_network(self, mode_subset=None, contact_cutoff=None, min_correlation=0.0):
        """Shortest communication paths and path usage of the ``dcc`` map (:func:`nma.correlation_network`)."""
        return nma.correlation_network(self, "dcc", mode_subset, contact_cutoff, min_correlation)

    def overlap(self, displacement, mode_subset=None):
        """Overlap of the selected modes with one or q displacements, (k,) / (q, k) (:func:`nma.overlap`)."""
        return nma.overlap(self, displacement, mode_subset)

    def distance_fluctuation(self, mode_subset=None, projected=True, tem=None, tem_factors=K_B):
        """Fluctuations of the inter-atom distances, (n, n) (:func:`nma.distance_fluctuation`; no reference counterpart)."""
        return nma.distance_fluctuation(self, mode_subset, projected, tem, tem_factors)

    def mode_displacement(self, coefficients, mode_subset=None):
        """Displacement field(s) (n,) / (q,n) ``sum_k c_k v_k`` over the selected modes (:func:`nma.mode_displacement`)."""
        return nma.mode_displacement(self, coefficients, mode_subset)

    def deformation_energy(self, mode_subset=None):
        """Per-atom deformation energies of the selected modes, (k, n); a row sums to its eigenvalue (:func:`nma.deformation_energy`)."""
        return nma.deformation_energy(self, mode_subset)

    def spring_strain(self, mode_subset=None):
        """(springs (P, 2), strain (k, P)): what every spring stores in the selected modes (:func:`nma.spring_strain`)."""
        return nma.spring_strain(self, mode_subset)

    def collectivity(self, mode_subset=None):
        """Collectivity of the selected modes, (k,) (:func:`nma.collectivity`)."""
        return nma.collectivity(self, mode_subset)

    def rmsip(self, other, n_modes=10, mode_subset=None):
        """RMSIP of this model's mode subspace with ``other``'s (:func:`nma.rmsip`; no reference counterpart)."""
        return nma.rmsip(self, other, n_modes, mode_subset)

    def covariance_overlap(self, other, mode_subset=None):
        """Covariance overlap (Hess 2002) of this model with ``other`` (:func:`nma.covariance_overlap`)."""
        return nma.covariance_overlap(self, other, mode_subset)

    def mode_overlap_matrix(self, other, mode_subset_a, mode_subset_b=None):
        """(k_a, k_b) overlaps of this model's listed modes with ``other``'s (:func:`nma.mode_overlap_matrix`)."""
        return nma.mode_overlap_matrix(self, other, mode_subset_a, mode_subset_b)

    def subsystem(self, system, device=None):
        """
        The modes of the ``system`` atoms inside their relaxing environment, a :class:`~springcraft_amd.Subsystem` (dim 1)
        built from this model's atoms, force field and masses (vibrational subsystem analysis; no reference counterpart).
        """
        from .subsystem import Subsystem

        return Subsystem(self._coord, self._ff, system, masses=self._masses, dim=1, device=device)
