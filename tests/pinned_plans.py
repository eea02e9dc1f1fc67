"""The launch plans of the 6-state model at 1024 nodes that the benchmark lines and the profiles quote, by batch size: held to the library
on the GPU (tests/test_gpu_parity.py) and to the host-only policy on the CPU (tests/test_pass_plan_cpu.py)."""

# the shapes the benchmark lines and the profiles quote, pinned: a policy change has to be made here as well as in plan_pass
PINNED_PLANS = {128: dict(sw=2, ksplit=1, k_tile=16, store_mode=1, block_order=1, piece=0), 1024: dict(sw=2, ksplit=1, k_tile=16, store_mode=2, piece=0),
                16: dict(sw=1, ksplit=4), 64: dict(sw=1, ksplit=2), 80: dict(sw=1, ksplit=1, k_tile=16), 112: dict(sw=2, ksplit=1, k_tile=16),
                320: dict(sw=2, ksplit=1, k_tile=16, block_order=150), 4096: dict(sw=2, k_tile=8, column_tiles=2, store_mode=2, piece=0), 256: dict(sw=2, k_tile=8), 512: dict(sw=2, k_tile=16)}
