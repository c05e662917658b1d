"""
:class:`ANM` — Anisotropic Network Model (host mirror of the reference's anm.py:20-445).
"""

from . import nma
from ._model import ElasticNetworkModel

__all__ = ["ANM"]

K_B = nma.K_B
N_A = nma.N_A


class ANM(ElasticNetworkModel):
    """
    Anisotropic Network Model.

    Parameters
    ----------
    atoms : AtomArray, shape=(n,) or ndarray, shape=(n,3), dtype=float
        The atoms (usually C-alpha only) or their coordinates.
    force_field : ForceField, natoms=n
    masses : bool or ndarray, shape=(n,), dtype=float, optional
        Mass-weight the Hessian with 1/sqrt(m_i m_j); ``True`` infers residue masses from
        ``atoms.res_name`` (needs an AtomArray).
    use_cell_list : bool, optional
        Interface compatibility only; the device contact scan does not need it.

    Attributes
    ----------
    hessian : ndarray, shape=(n*3,n*3), dtype=float
        Partitioned ``[x1, y1, z1, ... xn, yn, zn]``.  Not a copy.
    covariance : ndarray, shape=(n*3,n*3), dtype=float
        Pseudo-inverse of the Hessian.  Not a copy.
    masses : None or ndarray, shape=(n,), dtype=float
    """

    _dim = 3

    @property
    def hessian(self):
        return self._get_matrix()

    @hessian.setter
    def hessian(self, value):
        self._set_matrix(value, IndexError)

    @property
    def covariance(self):
        return self._get_covariance()

    @covariance.setter
    def covariance(self, value):
        self._set_covariance(value)

    def eigen(self, subset_by_index=None, subset_by_value=None):
        """
        Eigenvalues (ascending, shape (3n,)) and eigenvectors (rows, shape (3n,3n)) of the
        Hessian; the first six belong to rigid-body motions (anm.py:150-167).
        ``subset_by_index`` / ``subset_by_value``: a part of the spectrum only, see :func:`nma.eigen`.
        """
        return nma.eigen(self, subset_by_index, subset_by_value)

    def normal_mode(self, index, amplitude, frames, movement="sine"):
        """Displacements (frames, n, 3) animating mode ``index`` (anm.py:169-207)."""
        return nma.normal_mode(self, index, amplitude, frames, movement)

    def linear_response(self, force, mode_subset=None):
        """
        Displacement (n,3) induced by ``force`` via linear response theory (anm.py:209-238); q forces (q,n,3) give
        (q,n,3), ``mode_subset`` the response carried by those modes alone (:func:`nma.linear_response`).
        """
        return nma.linear_response(self, force, mode_subset)

    def mode_displacement(self, coefficients, mode_subset=None):
        """Displacement field(s) (n,3) / (q,n,3) ``sum_k c_k v_k`` over the selected modes (:func:`nma.mode_displacement`)."""
        return nma.mode_displacement(self, coefficients, mode_subset)

    def frequencies(self):
        """Mode frequencies in arbitrary units, ascending (anm.py:240-256)."""
        return nma.frequencies(self)

    def mean_square_fluctuation(self, mode_subset=None, tem=None, tem_factors=K_B):
        """Per-atom mean square fluctuation (anm.py:258-289)."""
        return nma.mean_square_fluctuation(self, mode_subset, tem, tem_factors)

    def bfactor(self, mode_subset=None, tem=None, tem_factors=K_B):
        """Isotropic B-factors from the MSF (anm.py:291-321)."""
        return nma.bfactor(self, mode_subset, tem, tem_factors)

    def dcc(self, mode_subset=None, norm=True, tem=None, tem_factors=K_B):
        """Dynamic cross-correlation (n,n) between nodes (anm.py:323-382)."""
        return nma.dcc(self, mode_subset, norm, tem, tem_factors)

    def anisotropic_fluctuation(self, mode_subset=None, tem=None, tem_factors=K_B):
        """Per-atom 3x3 fluctuation tensors (n,3,3) whose trace is the MSF (:func:`nma.anisotropic_fluctuation`)."""
        return nma.anisotropic_fluctuation(self, mode_subset, tem, tem_factors)

    def overlap(self, displacement, mode_subset=None):
        """Overlap of the selected modes with one or q displacements, (k,) / (q, k) (:func:`nma.overlap`)."""
        return nma.overlap(self, displacement, mode_subset)

    def distance_fluctuation(self, mode_subset=None, projected=True, tem=None, tem_factors=K_B):
        """Fluctuations of the inter-atom distances, (n, n) (:func:`nma.distance_fluctuation`; no reference counterpart)."""
        return nma.distance_fluctuation(self, mode_subset, projected, tem, tem_factors)

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

    def generalized_correlation(self, mode_subset=None, information=False):
        """Generalized correlation (n, n) from the linear mutual information (:func:`nma.generalized_correlation`)."""
        return nma.generalized_correlation(self, mode_subset, information)

    def correlation_network(self, kind="dcc", mode_subset=None, contact_cutoff=None, min_correlation=0.0):
        """Shortest communication paths and path usage of the ``dcc`` / ``lmi`` map (:func:`nma.correlation_network`)."""
        return nma.correlation_network(self, kind, mode_subset, contact_cutoff, min_correlation)

    def subsystem(self, system, device=None):
        """
        The modes of the ``system`` atoms inside their relaxing environment, a :class:`~springcraft_amd.Subsystem` built
        from this model's atoms, force field and masses (vibrational subsystem analysis; no reference counterpart).
        """
        from .subsystem import Subsystem

        return Subsystem(self._coord, self._ff, system, masses=self._masses, dim=3, device=device)

    def prs_effector_sensor(self, norm=True, mode_subset=None):
        """
        PRS matrix plus effector / sensor profiles (anm.py:384-445); ``mode_subset`` (extension): over the listed modes
        alone (:func:`nma.prs`).
        """
        prs_mat = nma.prs(self, norm, mode_subset)
        eff, sens = nma.effector_sensor(prs_mat)
        return prs_mat, eff, sens
