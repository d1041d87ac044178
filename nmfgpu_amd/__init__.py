"""nmfgpu_amd -- host-side Python mirror of the nmfgpu interface on top of libnmfgpu64.so.

The compute path is the C-ABI shared library built from nmfgpu_amd/csrc (hand-written gfx950
HIP kernels).  There is no Python, PyTorch or CPU fallback: importing the package works
anywhere (so that build and ABI checks can run without a GPU), but every compute entry point
raises / returns an error status when the library or a HIP device is missing.
"""
from ._lib import library, library_path, LibraryMissing  # noqa: F401
from .api import (  # noqa: F401
    ResultType, NmfInitializationMethod, NmfThresholdType, NmfAlgorithm, Verbosity, IndexBase, StorageFormat,
    ExecutionRecord, MatrixDescription, NmfDescription, Parameter, GpuInformation, KMeansDescription,
    initialize, finalize, version, choose_gpu, get_number_of_gpu, get_information_for_gpu_index,
    set_verbosity, compute, compute_kmeans, Summary, NmfError,
)
from .engine import device_matrix, device_vector, device_pointer_info, COLUMN_MAJOR, ROW_MAJOR  # noqa: F401
from .engine import Engine, EngineError, op_factor_product, op_factor_product_bf16, op_factor_product_x3, op_gram, op_gram_image, op_gram64_partials, op_gram_wide, split_image_bytes, op_inverse, inverse_padded_rank, op_factor_passes, op_tri_update, op_hals_sweep, op_hals_sweeps, op_hals_sweeps_dyn, op_apg_steps, op_apg_steps_dyn, op_hals_normalize, op_beta_half_step, op_beta_half_step_general, op_beta_half_step_weighted, op_beta_half_step_mixed, op_beta_update_rows, op_beta_fused, op_beta_update, op_kl_fused, op_masked_beta_half_step, op_masked_cd_half_step, missing_solver_fault, masked_norm_parts, op_predict_entries, predict_entry_parts, split_entries, op_top_k, top_k_slabs, TOPK_MAX_K, exclusion_lists, op_kl_update, op_kl_sums, op_panel_rowsum, op_spmm_rows, op_sddmm_quotient, op_panel_update, op_mu64_update, device_count, host_kmeans, host_init, RcclComm, LocalGroup, LocalComm, ShardedRun, shard_columns, SHARD_ROW_BLOCKS, SHARD_REPLICATED  # noqa: F401
