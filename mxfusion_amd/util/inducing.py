"""Inducing inputs from data: k-means centres of X (Lloyd iterations on the fused nearest-centre kernel, mxf_kmeans_step) or the rows that
greedily maximise the conditional prior variance (the pivoted-Cholesky selection of Burt et al. 2019, "Rates of convergence for sparse
variational Gaussian process regression").  No reference counterpart: the reference draws np.random.randn(num_inducing, Q) when the module is
defined, and so do the modules here; these helpers overwrite that draw in an initialised inference.

    infr.initialize(X=X.shape, Y=Y.shape)
    initialize_inducing_inputs(infr, m.Y, X)                  # k-means; method='greedy_variance' for the other
    infr.run(X=X, Y=Y, ...)

No sample axis: X is (N, Q) on the device, Q <= 16 for k-means (ops.nearest).  Hidden layers of a deep GP, whose inputs are not data, are out
of scope."""
import numpy as np
import torch

from .. import ops
from ..components.distributions.gp._iterative import pivoted_cholesky


def _check_X(what, X, M):
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError('%s: X is a (N, Q) tensor; got %s' % (what, tuple(X.shape) if hasattr(X, 'shape') else type(X).__name__))
    if int(M) < 1:
        raise ValueError('%s: M must be at least 1; got %d' % (what, M))
    return int(X.shape[0]), int(X.shape[1])


def kmeanspp_rows(X, M, seed=0):
    """The M rows of X (an int64 tensor on the host) that D^2 sampling (k-means++, Arthur & Vassilvitskii 2007) picks from M float64 uniforms
    u = numpy.random.RandomState(seed).random_sample(M): row floor(u_0 N), then searchsorted(cumsum(d2, float64), u_k total, right=True)
    clamped to N - 1, with d2 the running minimum squared distance to the rows chosen so far, exactly 0 at those rows."""
    N, Q = _check_X('kmeans++', X, M)
    u = np.random.RandomState(seed).random_sample(int(M))
    rows = [min(int(np.floor(u[0] * N)), N - 1)]
    d2 = ((X - X[rows[0]]) ** 2).sum(1)
    d2[rows[0]] = 0.0
    for k in range(1, int(M)):
        cs = torch.cumsum(d2.double(), 0)
        total = float(cs[-1])
        if total == 0.0:
            raise ValueError('kmeans++: X has only %d distinct rows, fewer than M = %d' % (k, M))
        target = torch.tensor([u[k] * total], dtype=torch.float64, device=X.device)
        r = min(int(torch.searchsorted(cs, target, right=True)), N - 1)
        rows.append(r)
        d2 = torch.minimum(d2, ((X - X[r]) ** 2).sum(1))
        d2[r] = 0.0
    return torch.as_tensor(rows, dtype=torch.int64)


def kmeans(X, M, num_iter=25, tol=1e-4, init='kmeans++', seed=0):
    """(Z, info): Z (M, Q) the k-means centres of X (N, Q) after at most num_iter Lloyd iterations, each one ops.kmeans_step call and one host
    read; it stops once the inertia's relative drop from one iteration to the next is <= tol.  init: 'kmeans++' (kmeanspp_rows), 'random'
    (the first M entries of numpy.random.RandomState(seed).permutation(N)) or a (M, Q) tensor.  A cluster that ends an iteration empty is
    re-seeded at the row farthest from its centre: the k-th empty cluster takes the row with the k-th largest distance.
    info: 'inertia' (a list: the sum of squared distances to the centres each iteration started from), 'counts' (M,) int64 of the last
    assignment, 'iterations', 'converged'."""
    N, Q = _check_X('kmeans', X, M)
    M = int(M)
    if Q > ops._lib.NEAREST_MAX_Q:
        raise ValueError('kmeans: Q = %d above the limit of %d input dimensions' % (Q, ops._lib.NEAREST_MAX_Q))
    X = X.detach().contiguous()
    if isinstance(init, torch.Tensor):
        if tuple(init.shape) != (M, Q):
            raise ValueError('kmeans: init is a (%d, %d) tensor; got %s' % (M, Q, tuple(init.shape)))
        C = init.detach().to(device=X.device, dtype=X.dtype).contiguous().clone()
    elif init == 'kmeans++':
        C = X[kmeanspp_rows(X, M, seed).to(X.device)].contiguous()
    elif init == 'random':
        if M > N:
            raise ValueError('kmeans: M = %d centres from N = %d rows' % (M, N))
        C = X[torch.as_tensor(np.random.RandomState(seed).permutation(N)[:M].astype(np.int64)).to(X.device)].contiguous()
    else:
        raise ValueError("kmeans: init is 'kmeans++', 'random' or a (M, Q) tensor; got %r" % (init,))
    info = dict(inertia=[], counts=torch.zeros(M, dtype=torch.int64, device=X.device), iterations=0, converged=False)
    for it in range(int(num_iter)):
        C_new, idx, counts, inertia = ops.kmeans_step(X, C)
        cur, n_empty = torch.stack([inertia, (counts == 0).sum().double()]).tolist()      # the iteration's one host read
        if n_empty:
            d2 = ((X - C[idx.long()]) ** 2).sum(1)
            far = torch.topk(d2, min(int(n_empty), N)).indices
            empty = torch.nonzero(counts == 0).reshape(-1)[:far.numel()]
            C_new[empty] = X[far]
        prev = info['inertia'][-1] if info['inertia'] else None
        info['inertia'].append(cur)
        info['counts'], info['iterations'] = counts, it + 1
        C = C_new
        if prev is not None and prev - cur <= tol * prev:
            info['converged'] = True
            break
    return C, info


def greedy_variance(X, kernel, M, **kernel_params):
    """(Z, idx): the M rows of X (N, Q), Z = X[idx], that greedily maximise the conditional prior variance k(x, x) - k(x, Z) K(Z, Z)^-1 k(Z, x)
    given the rows already taken -- the pivots of a rank-M pivoted Cholesky of K(X, X), which is never formed: one row of it per pivot
    (kernel.K) and its diagonal (kernel.Kdiag).  Any kernel; kernel_params are its parameters under their prefixed names
    (rbf_lengthscale=..., rbf_variance=...), with or without the sample axis.  idx is an int64 tensor on X's device, in the order taken."""
    N, Q = _check_X('greedy_variance', X, M)
    with torch.no_grad():
        Xs = X.detach().contiguous().unsqueeze(0)
        params = {}
        for n, v in kernel_params.items():
            v = torch.as_tensor(v).detach().to(device=X.device, dtype=X.dtype)
            params[n] = (v.reshape(1, -1) if v.dim() < 2 else v).contiguous()
        diag = kernel.Kdiag(None, Xs, **params)[0].contiguous()
        row = lambda i: kernel.K(None, Xs.index_select(1, i.reshape(1)), Xs, **params)[0, 0]
        _, idx = pivoted_cholesky(row, diag, M, return_pivots=True)
    if idx.numel() < int(M):
        raise ValueError('greedy_variance: only %d of the M = %d rows asked for have a conditional variance above 1e-12 of the largest prior '
                         'variance' % (idx.numel(), M))
    return X[idx], idx


def initialize_inducing_inputs(infr, variable, X, method='kmeans', **kw):
    """Sets the inducing inputs of the sparse GP module behind `variable` (its output variable: m.Y) in an initialised GradBasedInference
    `infr` to the k-means centres of X (method='kmeans', kw: num_iter, tol, init, seed) or to its greedy conditional-variance rows
    (method='greedy_variance', with the kernel parameters' current values in infr.params), in the parameter's dtype; returns the stored value."""
    factor = getattr(variable, 'factor', None)
    Zvar = getattr(factor, 'inducing_inputs', None)
    if Zvar is None:
        raise ValueError('initialize_inducing_inputs: the factor of the variable (%s) has no inducing_inputs: it is not a sparse GP module'
                         % type(factor).__name__)
    if not getattr(infr, '_initialized', False) or Zvar not in infr.params:
        raise ValueError('initialize_inducing_inputs: the inference is not initialised (or does not hold the inducing inputs as a parameter): '
                         'call infr.initialize(...) with the data shapes first')
    M, Q = (int(s) for s in infr.params[Zvar].shape)
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.shape[1] != Q:
        raise ValueError('initialize_inducing_inputs: X is (N, %d), the width of the inducing inputs (%d, %d); got %s'
                         % (Q, M, Q, tuple(X.shape) if hasattr(X, 'shape') else type(X).__name__))
    if method == 'kmeans':
        Z, _ = kmeans(X, M, **kw)
    elif method == 'greedy_variance':
        kernel = factor.kernel
        params = {n: infr.params[v] if v in infr.params else infr.params.constants[v.uuid] for n, v in kernel.parameters.items()}
        Z, _ = greedy_variance(X, kernel, M, **params, **kw)
    else:
        raise ValueError("initialize_inducing_inputs: method is 'kmeans' or 'greedy_variance'; got %r" % (method,))
    if tuple(Z.shape) != (M, Q):
        raise ValueError('initialize_inducing_inputs: %s gave %s where the inducing inputs are (%d, %d)' % (method, tuple(Z.shape), M, Q))
    infr.params[Zvar] = Z
    return infr.params[Zvar]
