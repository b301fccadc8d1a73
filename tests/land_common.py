"""Shared pieces of the land-elimination tests (test_gpu_land.py, test_gpu_passive_matrix.py): the cases, the model with land tiles skipped or not."""
BIG = {"POP_XCD_REMAP": "0"}     # the linear workgroup order the size rule gives above 2^19 columns (`wide` alone would get the XCD bands)
CASES = [
    ("wide", {"vmix_choice": 3, "hmix_momentum": 4, "hmix_tracer": 4, "am": -1.0e19, "ah": -1.0e18, "time_mix_freq": 5}, BIG, 14),
    ("wide", {"vmix_choice": 3, "hmix_momentum": 4, "hmix_tracer": 4, "am": -1.0e19, "ah": -1.0e18, "time_mix_freq": 5, "solver_choice": 2}, {}, 12),
    ("wide", {"block_size_x": 1056, "tadvect": 2, "vmix_choice": 2, "tmix_opt": 1, "time_mix_freq": 4}, BIG, 12),
    ("wide", {"time_mix_freq": 5}, {}, 10),                                                      # fused pcg on the compacted chunk list
    ("wide", {"block_size_x": 1056, "solver_choice": 2}, {}, 10),                                # two blocks: lists padded to one length
    # the large-grid forms of the fused pcg on the compacted list: block sums by their own launch, two chunks per workgroup in step A
    # (k_fpcg_a_pair), two cells per thread in step B; one block and two
    ("wide", {"time_mix_freq": 5}, {"POP_SOLVER_PRESUM": "1"}, 10),
    ("wide", {"block_size_x": 1056}, {"POP_SOLVER_PRESUM": "1"}, 8),
    ("wide", {"time_mix_freq": 5}, {"POP_SOLVER_PRESUM": "1", "POP_FPCG_A_PAIR": "0"}, 8),
    ("wide", {"solver_choice": 3, "time_mix_freq": 5}, {}, 10),                                 # P-CSI: land chunks of both ping-pong halves stay 0
    ("wide", {"solver_choice": 3, "precond_choice": 1, "block_size_x": 1056}, BIG, 8),           # P-CSI + EVP, two blocks, large-grid order
    ("test", {"vmix_choice": 3, "stepped_bathymetry": 1, "time_mix_freq": 6}, {}, 13),          # 96 blocks, many of them land
    ("gx3v7", {"tadvect": 3, "tmix_opt": 3}, {}, 10),
    ("tiny", {"solver_choice": 3, "hmix_momentum": 4, "hmix_tracer": 4, "am": -1.0e22, "ah": -1.0e21, "lvariable_hmix": 1}, {}, 10),
    # the buffers the fused del4 first Laplacians share with other kernel choices: forward elimination inside the tracer kernel (E, F
    # of the second tracer in S3c / S3d) and the in-line order (d2t / d2u aliased onto S3a / S3b, which KPP also uses as scratch)
    ("wide", {"vmix_choice": 3, "hmix_momentum": 4, "hmix_tracer": 4, "am": -1.0e19, "ah": -1.0e18, "time_mix_freq": 5},
     {"POP_D2T_FUSE": "1", "POP_TRACER_FWD": "1", "POP_REG_THOMAS_T": "0"}, 10),
    ("wide", {"vmix_choice": 3, "hmix_momentum": 4, "hmix_tracer": 4, "am": -1.0e19, "ah": -1.0e18, "time_mix_freq": 5},
     {"POP_DEL4_SIDE": "0", "POP_D2T_FUSE": "1"}, 10),
]


def model(pkg, monkeypatch, cfg, env, skip):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("POP_LAND_SKIP", "1" if skip else "0")
    monkeypatch.setenv("POP_LAND_FULL_STEPS", "4")
    return pkg.PopModel(cfg)
