"""dbcsr_amd -- MI355X-native block-sparse multiply behind DBCSR's interfaces.

Host side (Python) above the C-ABI shared library ``libdbcsr_acc_amd.so``
(HIP kernels for gfx950).  PyTorch is used for device memory, streams and
``torch.distributed`` only.  There is no CPU fallback: importing
:mod:`dbcsr_amd.lib` raises if the native library is missing.
"""
from .lib import load_library, library_path  # noqa: F401
from .operations import dbcsr_add, dbcsr_add_on_diag, dbcsr_dot, dbcsr_frobenius_norm, dbcsr_scale, dbcsr_trace  # noqa: F401
from .operations import (dbcsr_get_diag, dbcsr_gershgorin_norm, dbcsr_maxabs_norm, dbcsr_norm, dbcsr_norm_column,  # noqa: F401
                         dbcsr_norm_frobenius, dbcsr_norm_gershgorin, dbcsr_norm_maxabsnorm, dbcsr_scale_by_vector, dbcsr_set_diag)
from .operations import dbcsr_matvec, dbcsr_multiply_dense, dbcsr_multivec, dbcsr_rank_update  # noqa: F401
from .operations import dbcsr_get_block_diag, dbcsr_invert_block_diag, dbcsr_scale_by_block_diag  # noqa: F401
from .operations import dbcsr_create_from_dense, dbcsr_from_dense, dbcsr_to_dense  # noqa: F401
from .operations import dbcsr_copy, dbcsr_function_of_elements, dbcsr_hadamard_product  # noqa: F401
from .operations import (dbcsr_func_artanh, dbcsr_func_asin, dbcsr_func_cos, dbcsr_func_dcos, dbcsr_func_ddcos, dbcsr_func_ddsin,  # noqa: F401
                         dbcsr_func_ddtanh, dbcsr_func_dsin, dbcsr_func_dtanh, dbcsr_func_inverse, dbcsr_func_sin, dbcsr_func_tanh)
from .operations import (dbcsr_create_from_blocks, dbcsr_get_blocks, dbcsr_put_blocks, dbcsr_reserve_all_blocks,  # noqa: F401
                         dbcsr_reserve_blocks, dbcsr_reserve_diag_blocks)
from .csr import dbcsr_create_from_csr, dbcsr_csr_to_torch, dbcsr_from_csr, dbcsr_to_csr  # noqa: F401
from .reblock import dbcsr_merged_block_sizes, dbcsr_reblock, dbcsr_reblock_into, dbcsr_split_block_sizes  # noqa: F401
from .submatrix import SubmatrixPlan, dbcsr_submatrix_apply, dbcsr_submatrix_gather, dbcsr_submatrix_plan, dbcsr_submatrix_scatter  # noqa: F401
from .tensor import (DbcsrTensor, dbcsr_t_block_indices, dbcsr_t_contract, dbcsr_t_copy, dbcsr_t_copy_matrix_to_tensor,  # noqa: F401
                     dbcsr_t_copy_tensor_to_matrix, dbcsr_t_create, dbcsr_t_create_from_blocks, dbcsr_t_filter, dbcsr_t_get_blocks, dbcsr_t_put_blocks)

__all__ = ["load_library", "library_path", "dbcsr_reblock", "dbcsr_reblock_into", "dbcsr_merged_block_sizes", "dbcsr_split_block_sizes",
           "dbcsr_add", "dbcsr_scale", "dbcsr_add_on_diag", "dbcsr_trace", "dbcsr_dot", "dbcsr_frobenius_norm",
           "dbcsr_maxabs_norm", "dbcsr_gershgorin_norm", "dbcsr_norm", "dbcsr_norm_frobenius", "dbcsr_norm_maxabsnorm", "dbcsr_norm_gershgorin",
           "dbcsr_norm_column", "dbcsr_get_diag", "dbcsr_set_diag", "dbcsr_scale_by_vector", "dbcsr_matvec", "dbcsr_multivec", "dbcsr_rank_update",
           "dbcsr_multiply_dense",
           "dbcsr_get_block_diag", "dbcsr_invert_block_diag", "dbcsr_scale_by_block_diag", "dbcsr_to_dense", "dbcsr_from_dense", "dbcsr_create_from_dense",
           "dbcsr_hadamard_product", "dbcsr_copy", "dbcsr_function_of_elements", "dbcsr_func_inverse", "dbcsr_func_tanh", "dbcsr_func_dtanh",
           "dbcsr_func_ddtanh", "dbcsr_func_artanh", "dbcsr_func_sin", "dbcsr_func_dsin", "dbcsr_func_ddsin", "dbcsr_func_asin", "dbcsr_func_cos",
           "dbcsr_func_dcos", "dbcsr_func_ddcos",
           "dbcsr_reserve_blocks", "dbcsr_put_blocks", "dbcsr_get_blocks", "dbcsr_reserve_diag_blocks", "dbcsr_reserve_all_blocks",
           "dbcsr_create_from_blocks",
           "dbcsr_to_csr", "dbcsr_from_csr", "dbcsr_create_from_csr", "dbcsr_csr_to_torch",
           "SubmatrixPlan", "dbcsr_submatrix_plan", "dbcsr_submatrix_gather", "dbcsr_submatrix_scatter", "dbcsr_submatrix_apply",
           "DbcsrTensor", "dbcsr_t_create", "dbcsr_t_create_from_blocks", "dbcsr_t_block_indices", "dbcsr_t_put_blocks", "dbcsr_t_get_blocks", "dbcsr_t_copy",
           "dbcsr_t_copy_matrix_to_tensor", "dbcsr_t_copy_tensor_to_matrix", "dbcsr_t_filter", "dbcsr_t_contract"]
