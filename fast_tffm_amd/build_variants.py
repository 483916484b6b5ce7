"""Build variants of the HIP module (``python -m fast_tffm_amd.build_native --variant NAME``,
selected at run time with ``FM_HIP_VARIANT=NAME``): name -> extra hipcc flags.

One is kept: ``mfma``, the matrix-core fp8 forward (hip/fm_fwd_mfma.hip), a separate kernel with its own
GPU test, measured slower and kept out of the default module on purpose.  An A/B of a kernel change
against its predecessor is built on a branch (an entry here plus the switch it defines) and deleted with
the losing code path once the result is recorded under profiles/ (profiles/README.md lists the retired
switches).

Kept out of build_native.py because that file is part of every module's content hash: adding a
variant here leaves the other builds current (a variant's own flags are hashed into its build).
"""

HIP_VARIANTS: dict[str, list[str]] = {"mfma": ["-DFM_WITH_MFMA=1"]}
