// For the files that call rocBLAS / rocSOLVER on the context's handles (omc_ensure_blas, omc_ensure_aux: omc_common.h).
#pragma once
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include "omc_common.h"

#define OMC_BLAS_CHECK(expr)                                   \
  do {                                                         \
    rocblas_status _s = (expr);                                \
    if (_s != rocblas_status_success) {                        \
      omc_set_error(#expr, hipErrorUnknown);                   \
      return OMC_HIP_ERROR;                                    \
    }                                                          \
  } while (0)
