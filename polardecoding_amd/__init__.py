"""polardecoding_amd -- MI355X-native polar decoders (SC / BP / SCL / CRC-aided SCL / CRC-aided SC-Flip / soft-output SCAN / BP list).

The product is the C-ABI shared library ``polardecoding_amd/lib/libpolar_hip.so`` (include/polar_hip.h):
hand-written HIP kernels for gfx950.  This package is the thin host-side mirror of the reference's
per-frame decode functions (``SCdecode`` / ``BP`` / ``SCLdecode`` / ``CASCL``), plus torch plumbing for
device buffers and multi-GPU sharding.  There is no CPU fallback: everything raises if the HIP library
is missing.
"""
from .api import (ALGO_BP, ALGO_BPL, ALGO_CASCL, ALGO_SC, ALGO_SCAN, ALGO_SCF, ALGO_SCL, BP_STOP_G, BP_STOP_NONE, CRC6_TAPS, CRC24C_TAPS, F32, F64, Q8, q8_quantize,
                  FLAG_BP_CONVERGED, FLAG_CRC_PASS, FLAG_RERANK, FLAG_TIE, RM_NONE, RM_PUNCTURE, RM_REPEAT, RM_SHORT_LLR, RM_SHORTEN, BP, BPL, bpl_cyclic_graphs, CASCL, Codebook, Decoder, FLAG_NO_CODE, Group, PolarError, SCAN, SCdecode, SCFlip, DSCFlip, SCLdecode, decode, lib_path, load_crc_matrix, load_library,
                  construct_mc, construct_order, q_sequence, rm_info_order, rm_select_n, save_crc_matrix,
                  PAC, PCCASCL, dyn_pac, dyn_pc5g, pac_info_order, pac_precode, pac_taps, pac_unprecode, systematic_check)

__all__ = ["Decoder", "Codebook", "FLAG_NO_CODE", "Group", "SCdecode", "BP", "SCLdecode", "CASCL", "SCFlip", "DSCFlip", "SCAN", "BPL", "bpl_cyclic_graphs", "decode", "PolarError", "load_library", "lib_path",
           "q_sequence", "load_crc_matrix", "save_crc_matrix", "ALGO_SC", "ALGO_BP", "ALGO_SCL", "ALGO_CASCL", "ALGO_SCF", "ALGO_SCAN", "ALGO_BPL", "F64", "F32", "Q8", "q8_quantize", "CRC6_TAPS", "CRC24C_TAPS",
           "FLAG_TIE", "FLAG_CRC_PASS", "FLAG_RERANK", "FLAG_BP_CONVERGED", "BP_STOP_NONE", "BP_STOP_G",
           "rm_select_n", "rm_info_order", "construct_order", "construct_mc", "RM_NONE", "RM_REPEAT", "RM_PUNCTURE", "RM_SHORTEN", "RM_SHORT_LLR",
           "PAC", "PCCASCL", "dyn_pac", "dyn_pc5g", "pac_info_order", "pac_precode", "pac_taps", "pac_unprecode", "systematic_check"]
