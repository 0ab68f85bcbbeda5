"""GGN eigenvalues during backpropagation (API of ``vivit.linalg.eigvalsh``)."""
from typing import Any, Callable, Dict, List

from torch import Tensor
from torch.nn import Module, Parameter

from vivit_amd import kernels
from vivit_amd.linalg.utils import (
    get_closures,
    get_hook_for_groups,
    get_vivit_extension,
    parameter_side_symeig,
    use_parameter_side,
)
from vivit_amd.utils import delete_savefield
from vivit_amd.utils.checks import check_key_exists, check_subsampling_unique, check_unique_params
from vivit_amd.utils.gram import reshape_as_square
from vivit_amd.utils.hooks import ParameterGroupsHook
from vivit_amd.utils.solve_queue import SolveQueue


class EigvalshComputation:
    """Provide the extension and the extension hook that compute GGN eigenvalues.

    Same constructor, methods, parameter-group keys and error conventions as
    vivit/linalg/eigvalsh.py:20-237.  The loss must use ``reduction='mean'``.
    Data flow on the device: per parameter one SYRK (or the factorised Linear path) accumulated
    in place into the group's ``[n, n]`` Gram (beta = 1), then one values-only ``symeig``.
    """

    def __init__(self, subsampling: List[int] = None, mc_samples: int = 0, verbose: bool = False, side: str = "gram",
                 data_parallel: bool = False, process_group=None, batched_solve: bool = False):
        """``side`` (not in the reference): ``"auto"`` solves a group on its parameter side (``P x P``) when it has
        fewer parameters than Gram rows, ``"gram"`` always decomposes the Gram matrix like the reference.
        ``data_parallel`` / ``process_group`` (not in the reference): every rank back-propagated ITS batch shard; the
        Gram matrix of the global batch is assembled across ranks (vivit_amd.distributed.BatchShardedGram), the
        eigenvalues are those of the GGN of the mean loss over the global batch, identical on every rank.
        ``batched_solve`` (not in the reference): for block-diagonal curvature with many groups of one Gram size.  A
        group that is solved on the Gram side on one device is not solved in its hook; its Gram matrix is queued, and
        the queue goes through ``kernels.symeigvals_batched`` -- eight matrices of 193 <= n <= 1280 share one launch,
        one per XCD, where a single solve idles seven of the eight -- as soon as eight matrices of one size wait, and
        for the remainder on the first ``get_result``.  The eigenvalues are those of ``batched_solve=False`` bit for
        bit.  Parameter-side groups and ``data_parallel=True`` keep the immediate solve.  Which stream a flush runs on
        and how ``get_result`` is ordered behind it: :class:`vivit_amd.utils.solve_queue.SolveQueue`."""
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
        # filled by side effect during backpropagation, keyed by id(group)
        self._batch_size: Dict[int, int] = {}
        self._evals: Dict[int, Tensor] = {}
        self._batched_solve = bool(batched_solve) and not data_parallel
        # (device, n, stream) -> [(gram, group_id, scale)]: Gram matrices waiting for a batched solve
        self._queue = SolveQueue(self._solve_queued)
        self._pending = self._queue.pending

    def _solve_queued(self, items) -> List[Tensor]:
        """Solve the queued Gram matrices in one batched call, store the spectra (rows of the one tensor returned)."""
        W = kernels.symeigvals_batched([g for g, _, _ in items], overwrite=True)
        for row, (_, group_id, scale) in zip(W.unbind(0), items):
            # eigenvalues are homogeneous of degree one: the O(n) vector is scaled instead of the n x n Gram
            if scale is not None:
                row *= scale
            if self._verbose:
                print(f"Group {group_id}: Store 'gram_evals'")
            self._evals[group_id] = row
        return [W]

    def get_result(self, group: Dict) -> Tensor:
        """Eigenvalues (ascending) of the group's GGN block; KeyError if unavailable."""
        self._queue.flush_all()
        try:
            return self._evals[id(group)]
        except KeyError as e:
            raise KeyError("No results available for this group") from e

    def get_extension(self):
        """Extension to pass to ``with backpack(...)``."""
        return get_vivit_extension(self._subsampling, self._mc_samples)

    def get_extension_hook(self, param_groups: List[Dict]) -> Callable[[Module], None]:
        """Hook to pass as ``extension_hook``; groups need the ``'params'`` key."""
        self._check_param_groups(param_groups)
        hook = ParameterGroupsHook.from_functions(
            param_groups, self.get_param_computation(), self.get_group_hook(), self.get_accumulate()
        )
        return get_hook_for_groups(param_groups, self._batch_size, hook, verbose=self._verbose)

    def get_param_computation(self) -> Callable[[ParameterGroupsHook, Parameter], Tensor]:
        verbose, savefield, side, dp = self._verbose, self._savefield, self._side, self._dp

        def param_computation(self: ParameterGroupsHook, param: Parameter):
            """Gram of this parameter, added in-kernel to the group accumulator if there is one.

            Groups solved on the parameter side keep their factors alive instead (a list of parameters is
            accumulated) until the group hook forms the ``P x P`` block."""
            closures = get_closures(param, savefield)
            group = self.get_group(self._param_to_group[id(param)])
            C, N = closures["shape_cn"]
            if use_parameter_side(group["params"], C * N, side):
                return [param]
            gram_fn = closures["gram_mat"]
            existing = self.current_accumulation(param)
            if dp is not None:  # batch-sharded factors: block rows / parameter shards, assembled in the group hook
                from vivit_amd.distributed import BatchShardedGram

                acc = existing if existing is not None else BatchShardedGram(C, N, dp["group"])
                closures["dp_add"](acc)
                delete_savefield(param, savefield, verbose=verbose)
                return acc
            if existing is None:
                gram = gram_fn()
            else:
                gram_fn(out=existing, beta=1.0)
                gram = existing  # same object: tells ``accumulate`` the sum is already done
            delete_savefield(param, savefield, verbose=verbose)
            return gram

        return param_computation

    def get_accumulate(self) -> Callable[[ParameterGroupsHook, Tensor, Tensor], Tensor]:
        def accumulate(self: ParameterGroupsHook, existing, update):
            if isinstance(existing, list):  # parameter-side group: collect the parameters
                return existing + update
            # ``update`` already is ``existing`` (+= done by the kernel's beta = 1) on the fused path
            if update is existing:
                return update
            return existing.add_(update)

        return accumulate

    def get_group_hook(self) -> Callable[[ParameterGroupsHook, Tensor, Dict[str, Any]], None]:
        batch_sizes, subsampling = self._batch_size, self._subsampling
        evals, verbose, savefield = self._evals, self._verbose, self._savefield
        batched, queue = self._batched_solve, self._queue

        def group_hook(self: ParameterGroupsHook, accumulation: Tensor, group: Dict):
            group_id = id(group)
            if verbose:
                print(f"Group {group_id}: Delete 'batch_size'")
            batch_size = batch_sizes.pop(group_id)
            scale = None if subsampling is None else batch_size / len(subsampling)  # eigvalsh.py:217-219
            if isinstance(accumulation, list):  # parameter side: P x P block of the GGN, zero-padded spectrum
                gram_evals, _, _ = parameter_side_symeig(group["params"], savefield, eigenvectors=False)
                for param in accumulation:
                    delete_savefield(param, savefield, verbose=verbose)
            else:
                if not isinstance(accumulation, Tensor):  # data-parallel accumulator: assemble (collectives inside)
                    # each rank's factors carry 1/sqrt(N_local); N_local / N_ggn(global) turns the sum into the GGN of
                    # the mean loss over the global batch (covers sub-sampling: len(subsampling) x ranks = N_ggn)
                    scale = batch_size / accumulation.N
                    accumulation = accumulation.finalize()
                gram_mat = reshape_as_square(accumulation)
                if batched:
                    queue.add(gram_mat, (gram_mat.shape[0],), (gram_mat, group_id, scale))
                    return
                gram_evals, _ = kernels.symeig(gram_mat, eigenvectors=False, overwrite=True)
            # eigenvalues are homogeneous of degree one: the O(n) vector is scaled instead of the n x n Gram
            if scale is not None:
                gram_evals *= scale
            if verbose:
                print(f"Group {group_id}: Store 'gram_evals'")
            evals[group_id] = gram_evals

        return group_hook

    @staticmethod
    def _check_param_groups(param_groups: List[Dict]):
        check_key_exists(param_groups, "params")
        check_unique_params(param_groups)
