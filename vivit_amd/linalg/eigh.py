"""GGN eigenpairs during backpropagation (API of ``vivit.linalg.eigh``)."""
from typing import Any, Callable, Dict, Iterable, List, Tuple
from warnings import warn

import torch
from torch import Tensor
from torch.nn import Module, Parameter

from vivit_amd import kernels
from vivit_amd.linalg.utils import (
    get_closures,
    get_hook_for_groups,
    get_vivit_extension,
    normalize,
    parameter_side_symeig,
    use_parameter_side,
)
from vivit_amd.utils import delete_savefield
from vivit_amd.utils.checks import check_key_exists, check_subsampling_unique, check_unique_params
from vivit_amd.utils.gram import reshape_as_square
from vivit_amd.utils.hooks import ParameterGroupsHook
from vivit_amd.utils.solve_queue import SolveQueue


class EighComputation:
    """Provide the extension and the extension hook that compute GGN eigenpairs.

    Same surface as vivit/linalg/eigh.py:21-292: groups need ``'params'`` and ``'criterion'``
    (``Callable[[Tensor], List[int]]`` on the ascending eigenvalues); the result is
    ``(evals[K], [Tensor[K, *p.shape] for p in group['params']])`` with unit-norm eigenvectors.
    """

    def __init__(
        self,
        subsampling: List[int] = None,
        mc_samples: int = 0,
        verbose: bool = False,
        warn_small_eigvals: float = 1e-4,
        side: str = "gram",
        data_parallel: bool = False,
        process_group=None,
        batched_solve: bool = False,
    ):
        """``side`` (not in the reference): ``"auto"`` solves a group on its parameter side (``P x P``, eigenvectors
        directly in parameter space) when it has fewer parameters than Gram rows; ``"gram"`` = reference path.
        ``data_parallel`` / ``process_group`` (not in the reference): batch-sharded ranks, see
        :class:`vivit_amd.linalg.EigvalshComputation`; the back-projection ``V e`` is summed over the ranks'
        samples with one all-reduce of ``K P`` floats.
        ``batched_solve`` (not in the reference): for block-diagonal curvature with many groups of one Gram size.  A
        group that is solved on the Gram side on one device is not solved in its hook: its Gram matrix is built as usual
        and queued together with the group's ``V_mat_prod`` closures, and the queue goes through
        ``kernels.symeig_reduce_batched`` -- reduction, bisection, inverse iteration and back-transformation of eight
        matrices of 193 <= n <= 1280 in one launch each, where a loop of single solves leaves most of the chip idle --
        as soon as eight matrices of one size wait, and for the remainder on the first ``get_result``.  A flush runs:
        batched reduction, per group scaling and ``criterion``, batched select, per group back-projection, ``normalize``
        and the small-eigenvalue warning.  The eigenvalues are those of ``batched_solve=False`` bit for bit; the
        eigenvectors agree to rounding (another back-transformation kernel).  The save-fields are deleted in the hook
        either way.  The price: the factors of up to eight queued groups (kept alive by the closures) and their Gram
        matrices stay in memory until their flush, where the immediate path frees each group's factors in its hook.
        Parameter-side groups and ``data_parallel=True`` keep the immediate solve.  Which stream a flush runs on and how
        ``get_result`` is ordered behind it: :class:`vivit_amd.utils.solve_queue.SolveQueue`."""
        check_subsampling_unique(subsampling)
        use_parameter_side([], 1, side)  # validates ``side``
        if data_parallel and side != "gram":
            raise ValueError("data_parallel needs side='gram'")
        self._dp = {"group": process_group} if data_parallel else None
        self._side = side
        self._subsampling = subsampling
        self._mc_samples = mc_samples
        self._verbose = verbose
        self._savefield = self.get_extension().savefield
        self._warn_small_eigvals = warn_small_eigvals
        self._batch_size: Dict[int, int] = {}
        self._evals: Dict[int, Tensor] = {}
        self._evecs: Dict[int, List[Tensor]] = {}
        self._batched_solve = bool(batched_solve) and not data_parallel
        # (device, n, stream) -> [(gram, group_id, scale, criterion, V_mat_prod closures, (C, N))]
        self._queue = SolveQueue(self._solve_queued)
        self._pending = self._queue.pending

    _SMALL_WARNING = (
        "Some eigenvectors have small eigenvalues."
        + " Their parameter space transformation is numerically unstable."
        + " This can spoil orthogonality of eigenvectors."
        + " Maybe use a more restrictive eigenvalue filter criterion."
    )

    def _solve_queued(self, items) -> List[Tensor]:
        """Solve the queued Gram matrices in one batched two-phase call, store the eigenpairs and return their tensors."""
        plan = kernels.symeig_reduce_batched([it[0] for it in items], overwrite=True)
        rows, keeps = list(plan.evals.unbind(0)), []
        for row, (_, _, scale, criterion, _, _) in zip(rows, items):
            if scale is not None:  # eigh.py:245-246; eigenvectors are scale invariant
                row *= scale
            keeps.append(criterion(row))
        all_evecs = plan.select(keeps)
        del plan
        results = []
        for row, keep, gram_evecs, (_, group_id, _, _, v_mat_prods, (C, N)) in zip(rows, keeps, all_evecs, items):
            results += self._finish(group_id, row[keep], gram_evecs, C, N, v_mat_prods)
        return results

    def _finish(self, group_id: int, gram_evals: Tensor, gram_evecs: Tensor, C: int, N: int,
                v_mat_prods: Iterable[Callable[[Tensor], Tensor]], acc=None) -> List[Tensor]:
        """From the kept eigenpairs ``(gram_evals [K], gram_evecs [n, K])`` of a group's Gram matrix to its result:
        warn, back-project through one ``V_mat_prod`` per parameter, normalise, store; returns the stored tensors.

        ``v_mat_prods`` is consumed one product at a time, so a generator can free a factor right after its product.
        ``acc``: the :class:`BatchShardedGram` of a data-parallel group -- this rank applies the rows of V it owns."""
        if (gram_evals.abs() < self._warn_small_eigvals).any():
            warn(self._SMALL_WARNING)
        gram_evecs = gram_evecs.transpose(0, 1).reshape(-1, C, N)  # selectable via the first axis: [K, C, N] (eigh.py:265)
        if acc is not None:
            gram_evecs = acc.local_samples(gram_evecs, 2).contiguous()
        group_evecs = [v_mat_prod(gram_evecs) for v_mat_prod in v_mat_prods]
        normalize(group_evecs)
        self._evals[group_id] = gram_evals
        self._evecs[group_id] = group_evecs
        return [gram_evals] + group_evecs

    def get_result(self, group: Dict) -> Tuple[Tensor, List[Tensor]]:
        """``(evals, evecs)`` of the group's GGN block; KeyError if unavailable."""
        self._queue.flush_all()
        try:
            return self._evals[id(group)], self._evecs[id(group)]
        except KeyError as e:
            raise KeyError("No results available for this group") from e

    def get_extension(self):
        return get_vivit_extension(self._subsampling, self._mc_samples)

    def get_extension_hook(self, param_groups: List[Dict]) -> Callable[[Module], None]:
        self._check_param_groups(param_groups)
        hook = ParameterGroupsHook.from_functions(
            param_groups, self.get_param_computation(), self.get_group_hook(), self.get_accumulate()
        )
        return get_hook_for_groups(param_groups, self._batch_size, hook, verbose=self._verbose)

    def get_param_computation(self) -> Callable[[ParameterGroupsHook, Parameter], None]:
        def param_computation(self: ParameterGroupsHook, param: Parameter):
            """Nothing per parameter: the closures must stay alive until the group is complete."""
            return None

        return param_computation

    def get_accumulate(self) -> Callable[[ParameterGroupsHook, None, None], None]:
        def accumulate(self: ParameterGroupsHook, existing: None, update: None) -> None:
            return None

        return accumulate

    def get_group_hook(self) -> Callable[[ParameterGroupsHook, None, Dict[str, Any]], None]:
        batch_sizes, subsampling, savefield = self._batch_size, self._subsampling, self._savefield
        evals, evecs, verbose = self._evals, self._evecs, self._verbose
        warn_small_eigvals, side, dp = self._warn_small_eigvals, self._side, self._dp
        small_warning = self._SMALL_WARNING
        batched, queue, finish = self._batched_solve, self._queue, self._finish

        def group_hook(self: ParameterGroupsHook, accumulation: None, group: Dict[str, Any]) -> None:
            group_id = id(group)
            if verbose:
                print(f"Group {group_id}: Delete 'batch_size'")
            batch_size = batch_sizes.pop(group_id)

            C, N = get_closures(group["params"][0], savefield)["shape_cn"]
            if use_parameter_side(group["params"], C * N, side):
                # P x P block of the GGN: its eigenvectors are the parameter-space eigenvectors themselves
                all_evals, Q, cols = parameter_side_symeig(group["params"], savefield, eigenvectors=True)
                if subsampling is not None:
                    all_evals *= batch_size / len(subsampling)
                keep = group["criterion"](all_evals)
                keep_t = torch.as_tensor(keep, dtype=torch.long, device=all_evals.device)
                kept_evals = all_evals[keep_t]
                if (kept_evals.abs() < warn_small_eigvals).any():
                    warn(small_warning)
                # padded zeros (cols == -1) address the Gram matrix' exact null space: no GGN eigenvector belongs
                # to them, their rows stay zero (the reference returns a normalised noise vector there)
                vecs = torch.zeros((len(keep), Q.shape[0]), dtype=Q.dtype, device=Q.device)
                kept_cols = cols[keep_t]
                valid = kept_cols >= 0
                if bool(valid.any()):
                    vecs[valid] = Q[:, kept_cols[valid]].T
                group_evecs, off = [], 0
                for param in group["params"]:
                    numel = param.numel()
                    group_evecs.append(vecs[:, off : off + numel].reshape(len(keep), *param.shape).contiguous())
                    off += numel
                    delete_savefield(param, savefield, verbose=verbose)
                evals[group_id] = kept_evals
                evecs[group_id] = group_evecs
                return

            # Gram matrix, accumulated over the group's parameters inside the kernel (eigh.py:239-242)
            gram_mat, acc = None, None
            if dp is not None:  # batch-sharded ranks: assemble the global Gram matrix (collectives inside)
                from vivit_amd.distributed import BatchShardedGram, all_reduce_sum_

                acc = BatchShardedGram(C, N, dp["group"])
                for param in group["params"]:
                    get_closures(param, savefield)["dp_add"](acc)
                gram_mat = acc.finalize()
            else:
                for param in group["params"]:
                    gram_fn = get_closures(param, savefield)["gram_mat"]
                    gram_mat = gram_fn() if gram_mat is None else gram_fn(out=gram_mat, beta=1.0)
            C, N = gram_mat.shape[:2]

            if batched and acc is None:  # queue for the batched two-phase solve (the closures keep the factors alive)
                square = reshape_as_square(gram_mat)
                scale = None if subsampling is None else batch_size / len(subsampling)
                v_mat_prods = []
                for param in group["params"]:
                    v_mat_prods.append(get_closures(param, savefield)["V_mat_prod"])
                    delete_savefield(param, savefield, verbose=verbose)
                item = (square, group_id, scale, group["criterion"], v_mat_prods, (C, N))
                queue.add(square, (square.shape[0],), item)
                return

            # two launches around the criterion callback: reduction + all eigenvalues, then only the kept eigenvectors
            # (inverse iteration + back-transformation of K rows; the reference computes all n and slices, eigh.py:248-253)
            plan = kernels.symeig_reduce(reshape_as_square(gram_mat), overwrite=True)
            gram_evals = plan.evals
            if acc is not None:  # mean over the global batch (covers sub-sampling), see EigvalshComputation
                gram_evals *= batch_size / acc.N
            elif subsampling is not None:  # eigh.py:245-246; eigenvectors are scale invariant
                gram_evals *= batch_size / len(subsampling)

            keep = group["criterion"](gram_evals)
            gram_evals, gram_evecs = gram_evals[keep], plan.select(keep)
            del plan

            def v_mat_prods():  # one at a time: each parameter's factor is freed right after its product
                for param in group["params"]:
                    v_mat_prod = get_closures(param, savefield)["V_mat_prod"]
                    if acc is None:
                        yield v_mat_prod
                    else:  # every rank applied the rows of V it owns; one all-reduce per parameter sums them
                        yield lambda mat: all_reduce_sum_(v_mat_prod(mat).contiguous(), acc.group)
                    delete_savefield(param, savefield, verbose=verbose)

            finish(group_id, gram_evals, gram_evecs, C, N, v_mat_prods(), acc)

        return group_hook

    @staticmethod
    def _check_param_groups(param_groups: List[Dict]):
        check_key_exists(param_groups, "params")
        check_key_exists(param_groups, "criterion")
        check_unique_params(param_groups)
