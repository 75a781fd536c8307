"""Sampling operators on the GPU (``pycsou/linop/sampling.py:25-1058``).

``Masking`` (``sampling.py:125-196``), ``DownSampling`` (``sampling.py:199-391``) and
``SubSampling`` (``sampling.py:25-122`` -> ``pylops.Restriction``) keep the reference's
constructors, shape rules and errors.  The boolean mask / index list becomes int32 gather
indices and the inverse map once, on the host; forward and adjoint are the gather kernels
``pcs_gather`` / ``pcs_gather_or_zero`` (``csrc/sampling.hip``).

``Pooling`` (``sampling.py:394-536``) runs the fused block kernels ``pcs_pool_fwd`` / ``pcs_pool_adj``
(``csrc/pool.hip``).  ``NNSampling`` (``sampling.py:539-687``), ``GeneralisedVandermonde``
(``sampling.py:690-769``) and ``MappedDistanceMatrix`` (``sampling.py:772-1058``) do their set-up (k-d trees,
Python callables, matrix assembly) once on the host and are then a gather, a dense matrix or a CSR matrix
on the device (``pcs_csr_spmv``, ``csrc/spmv.hip``).  A ``'dask'`` ``MappedDistanceMatrix`` of one of the Green
functions of ``pycsou_amd.math.green`` assembles nothing: it is matrix-free on ``pcs_mdm_apply`` (``csrc/mdm.hip``).
"""

import numpy as np
import scipy.sparse as sparse
import torch
from scipy.spatial import cKDTree

from .. import _ops as O
from ..core.linop import LinearOperator
from .base import DenseLinearOperator, ExplicitLinearOperator


class _Gather(LinearOperator):
    """y = x[idx]; adjoint x = 0, x[idx] = y (repeated indices: the last one wins)."""

    def _set_indices(self, idx, n):
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if n >= 2 ** 31:
            raise NotImplementedError('sampling operators index with int32 (size < 2^31)')
        inv = np.full(n, -1, dtype=np.int32)
        inv[idx] = np.arange(idx.size, dtype=np.int32)  # NumPy fancy assignment: last wins
        self._idx_host, self._inv_host = idx.astype(np.int32), inv
        self._idx = self._inv = None

    def _dev(self):
        if self._idx is None:
            self._idx = torch.as_tensor(self._idx_host).to(O.device())
            self._inv = torch.as_tensor(self._inv_host).to(O.device())
        return self._idx, self._inv

    def _apply(self, t):
        return O.gather(t, self._dev()[0])

    def _adj(self, t):
        return O.gather_or_zero(t, self._dev()[1])


class Masking(_Gather):
    """``sampling.py:125-196``: extract the entries marked ``True`` in ``sampling_bool``."""

    def __init__(self, size, sampling_bool, dtype=np.float64):
        self.sampling_bool = np.asarray(sampling_bool).reshape(-1).astype(bool)
        self.input_size = size
        self.nb_of_samples = self.sampling_bool[self.sampling_bool == True].size  # noqa: E712
        if self.sampling_bool.size != size:
            raise ValueError('Invalid size of boolean sampling array.')
        super().__init__(shape=(self.nb_of_samples, self.input_size), dtype=dtype)
        self._set_indices(np.flatnonzero(self.sampling_bool), size)


class DownSampling(Masking):
    """``sampling.py:199-391``: keep one sample every ``downsampling_factor`` along every axis
    (or along ``axis``); ``output_shape`` as the reference computes it."""

    def __init__(self, size, downsampling_factor, shape=None, axis=None, dtype=np.float64):
        if type(downsampling_factor) is int:
            if (shape is not None) and (axis is None):
                self.downsampling_factor = len(shape) * (downsampling_factor,)
            else:
                self.downsampling_factor = (downsampling_factor,)
        else:
            self.downsampling_factor = tuple(downsampling_factor)
        if shape is not None:
            if size != np.prod(shape):
                raise ValueError(f'Array size {size} is incompatible with array shape {shape}.')
            if (axis is not None) and (axis > len(shape) - 1):
                raise ValueError(f'Array size {size} is incompatible with array shape {shape}.')
        if (shape is None) and (len(self.downsampling_factor) > 1):
            raise ValueError('Please specify an array shape for multidimensional downsampling.')
        elif (shape is not None) and (axis is None) and (len(shape) != len(self.downsampling_factor)):
            raise ValueError(f'Inconsistent downsampling factors {downsampling_factor} for array of shape {shape}.')
        self.input_size = size
        self.input_shape = shape
        self.axis = axis
        self.downsampling_mask = self.compute_downsampling_mask()
        if self.input_shape is None:
            self.output_shape = None
        elif len(self.downsampling_factor) > 1:
            self.output_shape = tuple(int(np.sum(np.arange(n) % f == 0))
                                      for n, f in zip(self.input_shape, self.downsampling_factor))
        else:
            out = list(self.input_shape)
            out[self.axis] = int(np.sum(np.arange(self.input_shape[self.axis]) % self.downsampling_factor[0] == 0))
            self.output_shape = tuple(out)
        super().__init__(size=self.input_size, sampling_bool=self.downsampling_mask, dtype=dtype)

    def compute_downsampling_mask(self):
        if self.input_shape is None:
            return (np.arange(self.input_size) % self.downsampling_factor[0]) == 0
        if len(self.downsampling_factor) > 1:
            mask = True
            for ax in range(len(self.input_shape)):
                keep = (np.arange(self.input_shape[ax]) % self.downsampling_factor[ax]) == 0
                keep = keep.reshape(keep.shape + (len(self.input_shape) - 1) * (1,))
                mask = mask * np.swapaxes(keep, 0, ax)
        else:
            mask = np.zeros(shape=self.input_shape, dtype=bool)
            mask = np.swapaxes(mask, 0, self.axis)
            mask[(np.arange(self.input_shape[self.axis]) % self.downsampling_factor[0]) == 0, ...] = True
            mask = np.swapaxes(mask, 0, self.axis)
        return np.asarray(mask).reshape(-1)


class SubSamplingOp(_Gather):
    """``pylops.Restriction(M, iava, dims, dir)``: ``x.take(iava, axis)`` (C order)."""

    def __init__(self, size, sampling_indices, shape=None, axis=0, dtype='float64'):
        iava = np.asarray(sampling_indices, dtype=np.int64).reshape(-1)
        dims = (size,) if shape is None else tuple(int(s) for s in shape)
        if int(np.prod(dims)) != size:
            raise ValueError('shape and size are not compatible')
        idx = np.arange(size, dtype=np.int64).reshape(dims).take(iava, axis=axis).reshape(-1)
        super().__init__(shape=(idx.size, size), dtype=np.dtype(dtype))
        self.sampling_indices, self.input_shape, self.axis = iava, shape, axis
        out = list(dims)
        out[axis] = iava.size
        self.output_shape = tuple(out)
        self._set_indices(idx, size)


def SubSampling(size, sampling_indices, shape=None, axis=0, dtype='float64'):
    """``pycsou/linop/sampling.py:25-122``."""
    return SubSamplingOp(size, sampling_indices, shape=shape, axis=axis, dtype=dtype)


class Pooling(LinearOperator):
    """``sampling.py:394-536``: sum or average over constant-size blocks tiling an array of ``shape``; a
    dimension that the block size does not divide is zero padded (``skimage.measure.block_reduce`` with
    ``cval=0``), so ``'mean'`` divides a partial block by the full block size too.

    Reference quirk, kept: ``adjoint`` is plain unpooling -- every cell of a block receives the block's value --
    in BOTH modes, with no division for ``'mean'``.  It is the transpose of the ``'sum'`` operator and therefore
    not the transpose of the ``'mean'`` operator (which would divide by ``prod(block_size)``).

    ``'average'`` passes the reference's check and then fails inside ``block_reduce``; here it raises
    ``ValueError`` at construction.  ``compute_lipschitz_cst`` is the closed form this forward / adjoint pair
    implies, ``sqrt(lambda_max(adjoint o forward))``: with ``c`` the largest number of real cells in a block,
    ``sqrt(c)`` for ``'sum'`` and ``sqrt(c / prod(block_size))`` for ``'mean'``.

    Arrays of 1 to 3 dimensions take one launch; beyond that one pass per pooled axis of the same kernels on
    the (outer, axis, inner) view, the mean scale applied once."""

    def __init__(self, shape, block_size, pooling_func='mean', dtype=np.float64):
        if len(shape) != len(block_size):
            raise ValueError(f'Inconsistent block size {block_size} for array of shape {shape}.')
        if pooling_func not in ['mean', 'sum', 'average']:
            raise ValueError('pooling_func must be one of: "mean" or "sum".')
        if pooling_func == 'average':
            raise ValueError('pooling_func="average" is accepted by the reference\'s check but not by its '
                             'block_reduce call; use "mean".')
        if any(int(b) != b or b < 1 for b in block_size):
            raise ValueError(f'Block sizes must be integers >= 1, got {block_size}.')
        self.input_shape = shape
        self.block_size = block_size
        self.pooling_func = np.mean if pooling_func == 'mean' else np.sum
        self.pooling_func_kwargs = None
        self._dims = tuple(int(n) for n in shape)
        self._block = tuple(int(b) for b in block_size)
        self._scale = 1.0 / float(np.prod(self._block)) if pooling_func == 'mean' else 1.0
        self.output_shape = self.get_output_shape()
        self.output_size = int(np.prod(self.output_shape).astype(int))
        self.input_size = int(np.prod(self.input_shape).astype(int))
        super().__init__(shape=(self.output_size, self.input_size), dtype=dtype)

    def get_output_shape(self):
        return O.pooled_shape(self._dims, self._block)

    def _axes(self):
        """The axes a per-axis composition passes over (at least one, so that the scale is applied)."""
        axes = [a for a, b in enumerate(self._block) if b > 1]
        return axes or [len(self._block) - 1]

    @staticmethod
    def _view(cur, a, n, b):
        """Axis ``a`` (``n`` samples, block ``b``) of an array of shape ``cur`` as a 3-D problem: (outer, axis,
        inner), or (1, outer, axis) for the last axis, which then is the contiguous one."""
        outer, inner = int(np.prod(cur[:a])), int(np.prod(cur[a + 1:]))
        return ((1, outer, n), (1, 1, b)) if inner == 1 else ((outer, n, inner), (1, b, 1))

    def _apply(self, t):
        if len(self._dims) <= 3:
            return O.pool(t, self._dims, self._block, self._scale)
        cur, axes = list(self._dims), self._axes()
        for a in axes:
            t = O.pool(t, *self._view(cur, a, cur[a], self._block[a]), self._scale if a == axes[-1] else 1.0)
            cur[a] = self.output_shape[a]
        return t

    def _adj(self, t):
        if len(self._dims) <= 3:
            return O.unpool(t, self._dims, self._block, 1.0)
        cur = list(self.output_shape)
        for a in self._axes():
            t = O.unpool(t, *self._view(cur, a, self._dims[a], self._block[a]), 1.0)
            cur[a] = self._dims[a]
        return t

    def compute_lipschitz_cst(self, **kwargs):
        cells = float(np.prod([min(n, b) for n, b in zip(self._dims, self._block)])) if self.input_size else 0.0
        self.lipschitz_cst = self.diff_lipschitz_cst = float(np.sqrt(cells * self._scale))


class NNSampling(LinearOperator):
    """``sampling.py:539-687``: sample a signal defined on a mesh of L points at the on-mesh nearest neighbours of
    M off-mesh locations.  ``compute_nn`` stays on the host (``cKDTree``, set-up only); the forward is the gather
    ``pcs_gather``; the adjoint is the reference's mean over the samples that share a neighbour, 0 elsewhere:
    an L x M CSR matrix with weights ``1 / count``, each row listing its samples in ascending order, applied
    with ``pcs_csr_spmv``.

    Reference quirk, kept: ``shape = (samples.size, L)`` although the vectors have M = ``samples.shape[0]``
    entries -- for samples of shape (6, 2) on a 24-point mesh the shape is (12, 24) while ``op(x)`` has 6
    entries and ``adjoint`` takes 6.

    ``compute_lipschitz_cst`` is 1 whenever there is a sample (``adjoint o forward`` is the indicator of the
    mesh points that have one)."""

    def __init__(self, samples, grid, dtype=np.float64):
        samples, grid = np.asarray(samples), np.asarray(grid)
        if samples.shape[-1] != grid.shape[-1]:
            raise ValueError(
                f'The samples have dimension {samples.shape[-1]} but the grid has dimension {grid.shape[-1]}.')
        self.samples = samples
        self.grid = grid.reshape(-1, grid.shape[-1])
        self.input_shape = self.grid.shape[:-1]
        self.input_size = int(np.prod(self.input_shape).astype(int))
        if self.input_size >= 2 ** 31:
            raise NotImplementedError('sampling operators index with int32 (size < 2^31)')
        self.compute_nn()
        super().__init__(shape=(self.samples.size, self.input_size), dtype=dtype)
        nn = np.asarray(self.nn_indices, dtype=np.int64).reshape(-1)
        count = np.bincount(nn, minlength=self.input_size)
        self._mean_mat = sparse.csr_matrix((1.0 / count[nn], (nn, np.arange(nn.size))),
                                           shape=(self.input_size, nn.size))
        self._mean_mat.sort_indices()
        self._idx_host, self._idx, self._mean = nn.astype(np.int32), None, {}

    def compute_nn(self):
        """On-grid nearest neighbours of the sampling locations (host)."""
        self.grid_tree = cKDTree(data=self.grid, compact_nodes=False, balanced_tree=False)
        self.nn_distances, self.nn_indices = self.grid_tree.query(self.samples, k=1, p=2, workers=-1)

    def _apply(self, t):
        if self._idx is None:
            self._idx = torch.as_tensor(self._idx_host).to(O.device())
        return O.gather(t, self._idx)

    def _adj(self, t):
        A = self._mean.get(t.dtype)
        if A is None:
            A = self._mean[t.dtype] = O.DeviceCSR(self._mean_mat, t.dtype)
        return O.spmv(A, t)

    def compute_lipschitz_cst(self, **kwargs):
        self.lipschitz_cst = self.diff_lipschitz_cst = 1.0 if self._idx_host.size else 0.0


class GeneralisedVandermonde(DenseLinearOperator):
    """``sampling.py:690-769``: the matrix ``[phi_k(z_l)]`` of a list of functions at the sampling locations,
    built on the host and held as a dense operator."""

    def __init__(self, samples, funcs, dtype=np.float64):
        self.samples = np.asarray(samples).reshape(-1)
        self.funcs = list(funcs)
        super().__init__(ndarray=self.get_generalised_vandermonde_matrix().astype(dtype), is_symmetric=False)

    def _map_func(self, f):
        return f(self.samples)

    def get_generalised_vandermonde_matrix(self):
        return np.stack(list(map(self._map_func, self.funcs)), axis=-1)


class MappedDistanceMatrix(ExplicitLinearOperator):
    """``sampling.py:772-1058``: the matrix ``[phi(d(z_l, x_k))]`` of a function of the radial (``ord``-norm)
    or zonal (inner product, clipped to [-1, 1]) distance between two point sets; ``samples2=None`` takes
    ``samples1`` twice and marks the operator symmetric.  The matrix is assembled once on the host:

    * ``'dense'``: exactly as the reference does, one call of ``function`` on the L x K distances.
    * ``'sparse'`` (needs ``max_distance``): the pairs within ``max_distance`` come from ``cKDTree.query_ball_tree``
      (honouring ``ord`` and ``eps``, the smaller tree querying the larger as in the reference), ``function``
      is applied in one vectorised call over all retained pairs, and the result is stored as a CSR matrix
      with sorted indices: a sparse operator on ``pcs_csr_spmv``.  ``n_jobs``, ``verbose`` and
      ``joblib_backend`` are accepted and unused.
    * ``'dask'`` (the default), the reference's memory-lean form.  With ``function`` one of the Green functions of
      ``pycsou_amd.math.green``, points of at most ``PCS_MDM_MAX_DIM`` coordinates and a float32 / float64 ``dtype``
      the operator is matrix-free (``matrix_free = True``, ``mat = None``, ``is_dask = True``): the two point sets
      are uploaded once per dtype and ``pcs_mdm_apply`` (``csrc/mdm.hip``) evaluates ``phi(d(z_l, x_k))`` in
      registers, forward and adjoint being the same kernel with the point sets exchanged -- O(L + K) memory.
      ``max_distance``, ``eps`` and ``chunks`` are ignored, as the reference's dask path ignores them.  With any
      other callable (a lambda cannot run on the device), a higher dimension or another dtype, dask not being a
      dependency of this package, the dense matrix is built instead and ``is_dask`` stays ``False``."""

    def __init__(self, samples1, function, samples2=None, mode='radial', max_distance=None, dtype=np.float64,
                 chunks='auto', operator_type='dask', verbose=True, n_jobs=-1, joblib_backend='loky', ord=2., eps=0):
        if mode not in ['radial', 'zonal']:
            raise ValueError('Supported modes are "radial" or "zonal".')
        if (operator_type == 'sparse') and (max_distance is None):
            raise ValueError('Specify a maximal distance for sparse format.')
        samples1 = np.asarray(samples1)
        self.max_distance = max_distance
        self.mode = mode
        self.function = function
        self.samples1 = samples1 if samples1.ndim > 1 else samples1[:, None]
        if samples2 is None:
            self.samples2 = self.samples1
        else:
            samples2 = np.asarray(samples2)
            self.samples2 = samples2 if samples2.ndim > 1 else samples2[:, None]
        symmetric = samples2 is None
        self.dtype = dtype
        self.chunks = chunks
        self.operator_type = operator_type
        self.verbose = verbose
        self.n_jobs = n_jobs
        self.joblib_backend = joblib_backend
        self.ord = ord
        self.eps = eps
        self.matrix_free = self._device_function_ok()
        if self.matrix_free:
            LinearOperator.__init__(self, shape=(self.samples1.shape[0], self.samples2.shape[0]), dtype=dtype,
                                    is_explicit=True, is_dense=False, is_sparse=False, is_dask=True,
                                    is_symmetric=symmetric)
            self.mat = None
            self._spec = function._device_spec()
            self._points, self._partials = {}, {}
            return
        if operator_type == 'sparse':
            self.is_symmetric = symmetric       # get_sparse_mdm shares the tree of a symmetric operator
            mat = self.get_sparse_mdm()
        elif operator_type in ('dask', 'dense'):
            mat = self.get_dense_mdm()
        else:
            raise ValueError(f'Unsupported operator type {operator_type}.')
        super().__init__(array=mat, is_symmetric=symmetric)

    def _device_function_ok(self):
        """Whether the operator is matrix-free: the 'dask' type, a Green function of this package (recognised by
        class, nothing else) whose parameters have a device form, points the kernels hold in registers, a dtype they compute in."""
        from ..math.green import GREEN_CLASSES
        try:
            dt = np.dtype(self.dtype)
        except TypeError:
            return False
        return (self.operator_type == 'dask' and isinstance(self.function, GREEN_CLASSES)
                and self.function._device_ok()
                and self.samples1.ndim == 2 and self.samples2.ndim == 2
                and 1 <= self.samples1.shape[1] == self.samples2.shape[1] <= O.MDM_MAX_DIM
                and dt in (np.dtype(np.float32), np.dtype(np.float64)))

    def _pts(self, dtype):
        """The two point sets on the device in ``dtype`` (one tensor when the operator is symmetric)."""
        p = self._points.get(dtype)
        if p is None:
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(  # noqa: E731
                device=O.device(), dtype=dtype).contiguous()
            p1 = up(self.samples1)
            p = self._points[dtype] = (p1, p1 if self.samples2 is self.samples1 else up(self.samples2))
        return p

    def _mdm(self, t, adjoint):
        p1, p2 = self._pts(t.dtype)
        P, Q = (p2, p1) if adjoint else (p1, p2)
        _, spg, ngroups, need = O.mdm_plan(P.shape[0], Q.shape[0])
        ws = self._partials.get(adjoint)
        if need and (ws is None or ws.numel() != need or ws.device != t.device):
            ws = self._partials[adjoint] = torch.empty(need, dtype=torch.float64, device=t.device)
        return O.mdm_apply(self._spec, self.mode, self.ord, P, Q, t.contiguous(), ws, (spg, ngroups))

    def _apply(self, t):
        return self._mdm(t, False) if self.matrix_free else super()._apply(t)

    def _adj(self, t):
        return self._mdm(t, True) if self.matrix_free else super()._adj(t)

    def _apply_cols(self, T, axis, adjoint=False):
        if self.matrix_free:       # the generic loop over the lines on the device
            return LinearOperator._apply_cols(self, T, axis, adjoint)
        return super()._apply_cols(T, axis, adjoint)

    def _apply_cols_acc(self, T, axis, adjoint, acc):
        if self.matrix_free:
            return LinearOperator._apply_cols_acc(self, T, axis, adjoint, acc)
        return super()._apply_cols_acc(T, axis, adjoint, acc)

    def _distances(self, a, b):
        if self.mode == 'radial':
            return np.linalg.norm(a - b, axis=-1, ord=self.ord)
        return np.clip(np.sum(a * b, axis=-1), a_min=-1, a_max=1)

    def get_sparse_mdm(self):
        tree1 = cKDTree(data=self.samples1, compact_nodes=False, balanced_tree=False)
        tree2 = tree1 if self.is_symmetric else cKDTree(data=self.samples2, compact_nodes=False, balanced_tree=False)
        by_col = self.samples2.shape[0] < self.samples1.shape[0]
        small, big = (tree2, tree1) if by_col else (tree1, tree2)
        neighbours = small.query_ball_tree(big, self.max_distance, p=self.ord, eps=self.eps)
        counts = np.fromiter((len(n) for n in neighbours), dtype=np.int64, count=len(neighbours))
        centre = np.repeat(np.arange(len(neighbours), dtype=np.int64), counts)
        other = np.fromiter((j for n in neighbours for j in n), dtype=np.int64, count=int(counts.sum()))
        rows, cols = (other, centre) if by_col else (centre, other)
        values = np.asarray(self.function(self._distances(small.data[centre], big.data[other])))
        mat = sparse.coo_matrix((values, (rows, cols)), shape=(self.samples1.shape[0], self.samples2.shape[0]),
                                dtype=self.dtype).tocsr()
        mat.sort_indices()
        return mat

    def get_dense_mdm(self):
        distances = self._distances(self.samples1[:, None, :], self.samples2[None, ...])
        return np.asarray(self.function(distances)).astype(self.dtype)
