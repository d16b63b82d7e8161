"""Native operators of the reference's ``basicsr/ops`` as HIP kernels, under the reference's module paths."""
