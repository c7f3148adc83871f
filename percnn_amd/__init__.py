"""percnn_amd -- MI355X-native (gfx950) fused Pi-block time stepping for PeRCNN.

Only the hot path of isds-neu/PeRCNN lives here: the per-step fixed-stencil Laplacian, the
parallel 1x1-conv branches whose Hadamard product is the reaction term, the explicit Euler
update, their adjoint, and the T-step rollout -- as hand-written HIP kernels behind a C-ABI
(``include/percnn_pi.h``), with drop-in ``RCNNCell`` / ``RCNN`` modules on top.

Layout:  ``csrc/`` HIP kernels + the C-ABI translation units (pi_abi.hip: base block, slabs, physics residual;
pi_host.hip: the host runtime they share -- option table, launch geometry, residency guard -- no kernel;
pi_s1_abi.hip: Stage-1 block on the matrix cores; pi_up3d_abi.hip: 3D IC-generator contraction; pi_disc_abi.hip: Stage-2 library moments; pi_lib_abi.hip: library cell) ->
``libpercnn_pi.so``;  ``_lib`` ctypes binding + build;  ``ops`` the registered ``torch.ops.percnn.*`` operators;
``functional`` raw calls + autograd front-end;  ``modules`` the reference's
module interface;  ``stage1`` the Stage-1 cell;  ``slab`` multi-GPU slab decomposition;  ``physics`` physics-residual
loss;  ``discovery`` Stage-2 library moments + STRidge;  ``library_cell`` Stage-3 cell over that library;  ``synthetic`` initial states for benchmarks / tests.
"""
from ._lib import build, lib, set_option, LIB_PATH  # noqa: F401
from .functional import (pi_step, pi_rollout, pack_params, contract_block, param_count, rollout_fwd_, rollout_bwd,  # noqa: F401
                         step_fwd, step_bwd, PiStepFunction, PiRolloutFunction, pi_step_batched, pi_rollout_batched,
                         pi_step_ensemble, pi_rollout_ensemble, pi_rollout_sqerr_batched, pi_rollout_sqerr_ensemble,
                         pi_rollout_obs_sqerr_batched, pi_rollout_obs_sqerr_ensemble)
from .modules import RCNNCell, RCNN, Upscaler, Stage3LambdaOmegaCell, Stage3BurgersCell, gs2d_cell, gs3d_cell, lo2d_cell, laplace_stencil, CellEnsemble  # noqa: F401

from . import ops  # noqa: F401  (registers torch.ops.percnn.*)
from . import slab, synthetic, physics, stage1, discovery  # noqa: F401
from .stage1 import Stage1Cell  # noqa: F401
from .physics import physics_loss_batched  # noqa: F401
from .discovery import LIBRARY_TERMS, LibraryMoments, row_class, library_moments, stridge, train_stridge, discover  # noqa: F401
from . import library_cell  # noqa: F401
from .library_cell import LibraryCell, LibraryEnsemble  # noqa: F401

__version__ = "0.1.0"
