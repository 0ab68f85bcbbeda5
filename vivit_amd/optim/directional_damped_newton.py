"""Directionally damped Newton steps from the low-rank GGN (API of
``vivit.optim.directional_damped_newton``, vivit/optim/directional_damped_newton.py:24-419)."""
from typing import Callable, Dict, List, Optional, Tuple

from torch import Tensor
from torch.nn import Module

from vivit_amd import kernels
from vivit_amd.linalg.utils import get_hook_for_groups
from vivit_amd.optim.directional_derivatives import (
    GramDirectionsQueue,
    accumulate_dot_products,
    apply_factor,
    dot_products,
    gram_space_directions,
)
from vivit_amd.optim.utils import get_batch_grad_extension, get_sqrt_ggn_extension
from vivit_amd.utils import delete_savefield
from vivit_amd.utils.checks import check_key_exists, check_subsampling_unique, check_unique_params
from vivit_amd.utils.hooks import ParameterGroupsHook

_SMALL_EVALS_NEWTON = (
    "Some eigenvalues are small. This can lead to numerical instabilities"
    + " in the directional gradients and the transformation into parameter"
    + " space because they require division by the eigenvalue square root."
    + " Maybe use a more restrictive eigenvalue filter criterion."
)


class DirectionalDampedNewtonComputation:
    r"""Provide extensions and the hook for directionally damped Newton steps

    .. math:: s = \sum_{k=1}^K \frac{-\gamma_k}{\lambda_k + \delta_k} e_k

    along the GGN eigenvectors :math:`e_k` selected by the group's ``'criterion'``, with
    directional damping :math:`\delta_k` from the group's ``'damping'`` callback
    ``(evals[K], evecs[n,K], gammas[N,K], lambdas[N,K]) -> [K]``.  ``get_result(group)`` returns
    the step in the format of ``group['params']``.  The loss must use ``reduction='mean'``.
    """

    def __init__(
        self,
        subsampling_grad: Optional[List[int]] = None,
        subsampling_ggn: Optional[List[int]] = None,
        mc_samples_ggn: Optional[int] = 0,
        verbose: Optional[bool] = False,
        warn_small_eigvals: float = 1e-4,
        factorised: bool = False,
        data_parallel: bool = False,
        process_group=None,
        batched_solve: bool = False,
    ):
        """Reference signature (vivit/optim/directional_damped_newton.py:39-83) plus four opt-in extensions:

        ``factorised``: Linear weights keep ``V_t = s (x) z`` and ``grad_batch = delta (x) z`` factorised
          (vivit/extensions/secondorder/vivit/linear.py:41-42) -- same step, no ``[C, N, out, in]`` tensors (the only
          way BASELINE config 5 fits: its materialised factor is 2.7 TB).
        ``data_parallel`` / ``process_group``: every rank of the (default) ``torch.distributed`` group ran the backward
          pass on ITS batch shard; the Gram matrix and ``V^T g`` are assembled across ranks
          (:class:`vivit_amd.distributed.BatchShardedGram`), eigensolve / gammas / lambdas run replicated, each rank
          back-projects its own samples and one all-reduce of ``P`` floats sums the step
          (directional_damped_newton.py:370-373).  The batch size used for the scalings is the global one.
        ``batched_solve``: for block-diagonal curvature with many groups of one Gram size (one group per layer).  A group
          whose dot products are complete is not solved in its hook but queued under ``(device, n, C, N_grad, stream)``; a
          queue goes through ``kernels.symeig_reduce_batched`` (eight matrices of 193 <= n <= 1280 share every launch of
          the eigensolver), one batched ``select`` and ONE ``kernels.gram_directions_batched`` launch for all gammas and
          lambdas -- where the immediate mode issues reduce, select and four small launches per group -- as soon as eight
          groups wait, and for the remainder on the first ``get_result``.  Then, per group as in the immediate mode: the
          small-eigenvalue warning, the ``damping`` callback, the coefficients and the back-projection through the factors
          (:class:`vivit_amd.optim.directional_derivatives.GramDirectionsQueue`).  The save-fields are deleted in the hook
          either way.  The price: the Gram matrices, ``V_t_g_n`` AND the factors ``V`` of up to eight queued groups per
          size stay in memory until their flush, where the immediate mode frees each group's factors in its hook.  The
          steps agree with the immediate mode to rounding (the eigenvalues bit for bit; the eigenvectors come from
          another back-transformation kernel, their sign cancels in the step).  ``data_parallel=True`` keeps the
          immediate path.  Streams: :class:`vivit_amd.utils.solve_queue.SolveQueue`.
        """
        check_subsampling_unique(subsampling_grad)
        check_subsampling_unique(subsampling_ggn)
        self._mc_samples_ggn = mc_samples_ggn
        if self._mc_samples_ggn != 0:
            assert mc_samples_ggn == 1
        self._subsampling_grad = subsampling_grad
        self._subsampling_ggn = subsampling_ggn
        self._factorised = factorised
        self._dp = {"group": process_group} if data_parallel else None
        self._savefield_grad = get_batch_grad_extension(None).savefield
        self._savefield_ggn = get_sqrt_ggn_extension(None, mc_samples_ggn).savefield
        self._verbose = verbose
        self._warn_small_eigvals = warn_small_eigvals
        self._batch_size: Dict[int, int] = {}
        self._newton_steps: Dict[int, Tuple[Tensor]] = {}
        self._batched_solve = bool(batched_solve) and not data_parallel
        self._queue = GramDirectionsQueue(self._step, warn_small_eigvals, _SMALL_EVALS_NEWTON, verbose)

    def get_result(self, group: Dict) -> Tuple[Tensor]:
        self._queue.flush_all()
        try:
            return self._newton_steps[id(group)]
        except KeyError as e:
            raise KeyError("No results available for this group") from e

    def get_extensions(self) -> List:
        return [
            get_batch_grad_extension(self._subsampling_grad, factorised=self._factorised),
            get_sqrt_ggn_extension(subsampling=self._subsampling_ggn, mc_samples=self._mc_samples_ggn,
                                   factorised=self._factorised),
        ]

    def get_extension_hook(self, param_groups: List[Dict]) -> Callable[[Module], None]:
        self._check_param_groups(param_groups)
        hook = ParameterGroupsHook.from_functions(
            param_groups,
            lambda hook, param: self._param_computation(
                hook, param, self._savefield_ggn, self._savefield_grad, self._verbose, self._dp
            ),
            lambda hook, accumulation, group: (self._queue_group if self._batched_solve else self._group_hook)(
                accumulation, group
            ),
            lambda hook, existing, update: accumulate_dot_products(existing, update, self._verbose),
        )
        return get_hook_for_groups(param_groups, self._batch_size, hook, verbose=self._verbose)

    @staticmethod
    def _param_computation(hook, param, savefield_ggn, savefield_grad, verbose, data_parallel=None):
        result = dot_products(hook, param, savefield_ggn, savefield_grad, verbose, data_parallel)
        # V is kept for the back-projection of the step (directional_damped_newton.py:258)
        delete_savefield(param, savefield_grad, verbose=verbose)
        return result

    def _queue_group(self, accumulation, group):
        """``batched_solve``: queue the group with its factors (the queue keeps them alive), free the save-fields now."""
        factors = []
        for param in group["params"]:
            factors.append(getattr(param, self._savefield_ggn))
            delete_savefield(param, self._savefield_ggn, verbose=self._verbose)
        self._queue.add(accumulation, group, self._batch_size.pop(id(group)), payload=factors)

    def _group_hook(self, accumulation, group):
        """The immediate mode: directions, step and the end of the factors' save-fields in the group's hook."""
        N = self._batch_size.pop(id(group))
        *directions, dp_acc = gram_space_directions(
            accumulation, group, N, self._verbose, self._warn_small_eigvals, _SMALL_EVALS_NEWTON
        )
        params = group["params"]
        self._step(group, [getattr(param, self._savefield_ggn) for param in params], *directions, dp_acc=dp_acc)
        for param in params:
            delete_savefield(param, self._savefield_ggn, verbose=self._verbose)

    def _step(self, group, factors, evals, evecs, gammas, lambdas, V_correction, C, N_ggn, dp_acc=None) -> List[Tensor]:
        """From a group's directions (:func:`gram_space_directions` or the queue's flush) and the factors of its
        parameters to its Newton step: stored, and returned as the list of its tensors."""
        # coefficients along the directions (directional_damped_newton.py:353-359): O(K) glue
        coefficients = (
            -gammas.mean(0) / (lambdas.mean(0) + group["damping"](evals, evecs, gammas, lambdas)) / evals.sqrt()
        )
        # weight in Gram space (:362-366), then apply V (K7, :370-373): step_p = v^T V_p
        v = kernels.gemm_nn(evecs, coefficients.reshape(-1, 1).contiguous(), alpha=V_correction)  # [n, 1]
        coef = v.reshape(1, C, N_ggn)
        if dp_acc is not None:
            # data parallel: this rank applies the rows of V it owns, one all-reduce of P floats sums the shards
            from vivit_amd.distributed import all_reduce_sum_

            coef = dp_acc.local_samples(coef, 2).contiguous()
        steps = []
        for V, param in zip(factors, group["params"]):
            step = apply_factor(V, coef)[0]
            if dp_acc is not None:
                all_reduce_sum_(step, dp_acc.group)
            steps.append(step.view(param.shape))
        self._newton_steps[id(group)] = steps
        return steps

    @staticmethod
    def _check_param_groups(param_groups: List[Dict]):
        check_key_exists(param_groups, "params")
        check_key_exists(param_groups, "criterion")
        check_key_exists(param_groups, "damping")
        check_unique_params(param_groups)
