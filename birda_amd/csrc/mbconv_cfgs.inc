// (three parts, one translation unit each per activation -- MB_PART 0: entries 0-210, the hand-shaped ones; 1: 211-268, the generic
//  classes; 2: 269-300, the late-stage whole-image and E1 entries -- so that the 1 050 instantiations build on nine cores at once)
#if MB_PART == 0
// Tile configurations of the fused MBConv kernel (kernels_mbconv_<activation>.hip include this list once each, with MB_A set).
// MB_ENTRY* rows are the product: exactly the configurations mb_plan() reaches for the BirdNET-v2.4-shaped, Perch-sized (B3) and
// Perch-shaped (B0) stacks and the small test models in the three precisions (tools/plan_models.py;
// tests/test_abi_and_host.py::test_shipped_tile_configurations_are_the_reachable_ones holds the list to that).  MB_NONE / MB_NONE2 rows
// hold the place of measured alternatives that lost (DESIGN.md sections 3 and 8 have the numbers, and the table of section 8 the
// commit that last held their code): indices are ABI, so the place stays and matches no block.
//        KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC
    MB_NONE,    // 0: lost -- was 16 -> 96 -> 24, 48x256 -> 24x128
    MB_NONE,    // 1: lost -- was 24 -> 144 -> 24, 24x128
    MB_NONE,    // 2: lost -- was 24 -> 144 -> 40, 24x128 -> 12x64
    MB_ENTRY(5, 1, 48, 3, 4, 1, 4, 1, 3, 3, 4, 2, 12, 1, 1),   // 3: 40 -> 240 -> 40, 12x64, full-height tiles
    MB_NONE,    // 4: lost -- was 40 -> 240 -> 80, 12x64 -> 6x32
    MB_ENTRY(3, 1, 32, 5, 3, 1, 4, 1, 3, 5, 5, 1, 6, 1, 2),    // 5: 80 -> 480 -> 80, 6x32 whole image
    MB_ENTRY(5, 1, 32, 5, 3, 1, 4, 1, 3, 7, 5, 1, 6, 1, 1),    // 6: 80 -> 480 -> 112, 6x32
    MB_ENTRY(5, 1, 32, 7, 3, 1, 4, 1, 3, 7, 5, 1, 6, 1, 1),    // 7: 112 -> 672 -> 112, 6x32
    MB_ENTRY(5, 2, 32, 7, 3, 1, 1, 4, 3, 3, 4, 1, 3, 1, 1),    // 8: 112 -> 672 -> 192, 6x32 -> 3x16
    MB_ENTRY(5, 1, 32, 12, 3, 2, 2, 2, 3, 6, 4, 2, 3, 2, 1),   // 9: 192 -> 1152 -> 192, 3x16 x 2 segments
    MB_ENTRY(3, 1, 32, 12, 3, 2, 2, 2, 3, 10, 4, 2, 3, 2, 1),  // 10: 192 -> 1152 -> 320, 3x16 x 2 segments
    // 16-channel chunks: a quarter of the LDS, so 2-4 workgroups share a CU and overlap their phases
    MB_ENTRY(3, 2, 16, 1, 5, 1, 4, 1, 1, 2, 4, 0, 4, 1, 4),    // 11: as 0
    MB_ENTRY(3, 1, 16, 2, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 3),    // 12: as 1
    MB_ENTRY(5, 2, 16, 2, 7, 1, 4, 1, 1, 3, 4, 0, 4, 1, 2),    // 13: as 2
    MB_ENTRY(5, 1, 16, 3, 4, 1, 4, 1, 3, 3, 4, 2, 12, 1, 2),   // 14: as 3
    MB_ENTRY(3, 2, 16, 3, 7, 1, 2, 2, 3, 3, 4, 1, 6, 1, 2),    // 15: as 4
    MB_ENTRY(3, 1, 16, 5, 3, 1, 4, 1, 3, 5, 5, 2, 6, 1, 2),    // 16: as 5
    MB_ENTRY(5, 1, 16, 5, 3, 1, 4, 1, 3, 7, 5, 2, 6, 1, 2),    // 17: as 6
    MB_ENTRY(5, 1, 16, 7, 3, 1, 4, 1, 3, 7, 5, 2, 6, 1, 2),    // 18: as 7
    MB_ENTRY(5, 2, 16, 7, 3, 1, 1, 4, 3, 3, 4, 0, 3, 1, 2),    // 19: as 8
    // stem conv (im2col gather from the planar spectrogram) -> depthwise 3x3 -> project: the first block
    MB_ENTRY_S(3, 1, 16, 2, 3, 1, 4, 1, 2, 1, 4, 1, 8, 1, 3, 2),  // 20: 2-channel spectrogram, 3x3 stem (K = 18)
    MB_ENTRY_S(3, 1, 16, 1, 3, 1, 4, 1, 2, 1, 4, 1, 8, 1, 3, 1),  // 21: 1-channel spectrogram (K = 9)
    // f16 MFMA twins (even index: split hi/lo x3, odd: plain f16), 32-channel chunks
    //         KS ST KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM
    MB_NONE, MB_ENTRY_P(3, 2, 32, 1, 5, 1, 4, 1, 1, 2, 4, 1, 4, 1, 2, 0, 1),    // 22/23: Cin <= 32, 3x3 s2 (16 -> 96 -> 24); the split-f16 twin lost
    MB_NONE, MB_ENTRY_P(3, 1, 32, 1, 3, 1, 4, 1, 2, 2, 4, 2, 8, 1, 2, 0, 1),    // 24/25: Cin <= 32, 3x3 s1; the split-f16 twin lost
    MB_NONE, MB_ENTRY_P(5, 2, 32, 1, 7, 1, 4, 1, 1, 3, 4, 1, 4, 1, 2, 0, 1),    // 26/27: Cin <= 32, 5x5 s2; the split-f16 twin lost
    MB_NONE, MB_ENTRY_P(5, 1, 32, 2, 4, 1, 4, 1, 3, 3, 4, 3, 12, 1, 1, 0, 1),    // 28/29: Cin <= 64, 5x5 s1, 12x64; the split-f16 twin lost
    MB_NONE, MB_ENTRY_P(3, 2, 32, 2, 7, 1, 2, 2, 3, 3, 4, 0, 6, 1, 1, 0, 1),    // 30/31: Cin <= 64, 3x3 s2; the split-f16 twin lost
    MB_NONE, MB_ENTRY_P(3, 1, 32, 3, 3, 1, 4, 1, 3, 5, 5, 3, 6, 1, 2, 0, 1),    // 32/33: 80 -> 480 -> 80, 6x32; the split-f16 twin lost
    MB_NONE, MB_ENTRY_P(5, 1, 32, 3, 3, 1, 4, 1, 3, 7, 5, 3, 6, 1, 1, 0, 1),    // 34/35: 80 -> 480 -> 112; the split-f16 twin lost
    MB_NONE, MB_ENTRY_P(5, 1, 32, 4, 3, 1, 4, 1, 3, 7, 5, 3, 6, 1, 1, 0, 1),    // 36/37: 112 -> 672 -> 112; the split-f16 twin lost
    MB_NONE, MB_ENTRY_P(5, 2, 32, 4, 3, 1, 1, 4, 3, 3, 4, 1, 3, 1, 1, 0, 1),    // 38/39: 112 -> 672 -> 192 stride 2; the split-f16 twin lost
    MB_ENTRY_H(5, 1, 6, 3, 2, 2, 2, 3, 6, 4, 2, 3, 2, 1, 0),    // 40/41: 192 -> 1152 -> 192, 3x16 x 2
    MB_ENTRY_H(3, 1, 6, 3, 2, 2, 2, 3, 10, 4, 2, 3, 2, 1, 0),   // 42/43: 192 -> 1152 -> 320
    MB_NONE, MB_ENTRY_P(3, 1, 32, 1, 3, 1, 4, 1, 2, 1, 4, 2, 8, 1, 2, 2, 1),    // 44/45: stem (2-channel spectrogram) block; the split-f16 twin lost
    MB_NONE, MB_ENTRY_P(3, 1, 32, 1, 3, 1, 4, 1, 2, 1, 4, 2, 8, 1, 2, 1, 1),    // 46/47: stem (1-channel spectrogram) block; the split-f16 twin lost
    // split-f16 with 16-channel chunks (k of the project GEMM zero-padded to 32): the large early images
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_ENTRY_P(3, 2, 16, 1, 5, 1, 4, 1, 1, 2, 4, 0, 4, 1, 4, 0, 3),    // 48: as 11
    MB_ENTRY_P(3, 1, 16, 1, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 3, 0, 3),    // 49: as 12
    MB_ENTRY_P(5, 2, 16, 1, 7, 1, 4, 1, 1, 3, 4, 0, 4, 1, 2, 0, 3),    // 50: as 13
    MB_ENTRY_P(5, 1, 16, 2, 4, 1, 4, 1, 3, 3, 4, 2, 12, 1, 2, 0, 3),   // 51: as 14
    MB_ENTRY_P(3, 2, 16, 2, 7, 1, 2, 2, 3, 3, 4, 1, 6, 1, 2, 0, 3),    // 52: as 15
    MB_NONE,    // 53: lost -- was as 20 (2-channel stem)
    MB_NONE,    // 54: lost -- was as 21 (1-channel stem)
    MB_ENTRY_P(3, 1, 16, 3, 3, 1, 4, 1, 3, 5, 5, 2, 6, 1, 2, 0, 3),    // 55: as 16 (80 -> 480 -> 80, 6x32)
    MB_NONE,    // 56: lost -- was as 17
    MB_NONE,    // 57: lost -- was as 18 (112 -> 672 -> 112)
    MB_ENTRY_P(5, 2, 16, 4, 3, 1, 1, 4, 3, 3, 4, 0, 3, 1, 2, 0, 3),    // 58: as 19
    // half-image tiles (3x32 of a 6x32 image) for the 5x5 blocks: 1.67x the expand work (cheap on the f16
    // MFMA) buys two or three workgroups per CU, whose phases then overlap
    MB_ENTRY_P(5, 1, 16, 4, 3, 1, 2, 2, 3, 4, 5, 2, 3, 1, 2, 0, 3),    // 59: 112 -> 672 -> 112
    MB_ENTRY_P(5, 1, 16, 3, 3, 1, 2, 2, 3, 4, 5, 2, 3, 1, 2, 0, 3),    // 60: 80 -> 480 -> 112
    // 32-wide tiles for the large early images: half the workgroups, half the per-workgroup set-up
    MB_NONE,    // 61: lost -- was as 48, tile 4x32
    MB_NONE,    // 62: lost -- was as 49, tile 8x32
    MB_NONE,    // 63: lost -- was as 20 (stem, f32), tile 8x32
    // four workgroups per CU for the gather-latency-bound stem block
    MB_NONE,    // 64: lost -- was as 20, 4 waves per SIMD
    MB_ENTRY_P(3, 1, 16, 1, 3, 1, 4, 1, 2, 1, 4, 1, 8, 1, 4, 2, 3),    // 65: as 53, 4 waves per SIMD
    MB_ENTRY_P(3, 1, 16, 1, 3, 1, 4, 1, 2, 1, 4, 1, 8, 1, 4, 1, 3),    // 66: as 54, 4 waves per SIMD
    // 16-channel chunks for the 3x16 blocks: with the 16-deep project step the workgroup needs < 80 KB of LDS,
    // so two share a CU
    MB_NONE,    // 67: lost -- was as 40 (192 -> 1152 -> 192, 3x16 x 2)
    MB_NONE,    // 68: lost -- was as 42 (192 -> 1152 -> 320)
    MB_NONE,    // 69: lost -- was as 48, tile 8x16 (17x33 source rows: 10 % halo; the one entry whose last expand group is a single row tile)
    // whole-image tiles for the Perch-shaped stack (128 mel x 497 frames -> 8x32 and 4x16 images in the late stages)
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_ENTRY_P(3, 1, 16, 3, 4, 1, 4, 1, 4, 5, 5, 2, 8, 1, 1, 0, 3),    // 70: 80 -> 480 -> 80, 8x32
    //         KS ST KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM
    MB_NONE2,    // 71/72: lost -- was 80 -> 480 -> 112, 8x32
    MB_ENTRY_H(5, 1, 4, 4, 1, 4, 1, 4, 7, 5, 3, 8, 1, 1, 0),           // 73/74: 112 -> 672 -> 112, 8x32
    MB_NONE2,    // 75/76: lost -- was 192 -> 1152 -> 192, 4x16 (one segment: no spills)
    MB_NONE2,    // 77/78: lost -- was 192 -> 1152 -> 320, 4x16
    // persistent twins of the early-block entries (48, 49, 65, 66, 50, 51): indices 79..84
    //          KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_NONE,    // 79: lost -- was as 48 (16 -> 96 -> 24, 48x256 -> 24x128)
    MB_NONE,    // 80: lost -- was as 49 (24 -> 144 -> 24, 24x128)
    MB_NONE,    // 81: lost -- was as 65 (stem block, 2-channel spectrogram)
    MB_NONE,    // 82: lost -- was as 66 (stem block, 1-channel spectrogram)
    MB_NONE,    // 83: lost -- was as 50 (24 -> 144 -> 40, 5x5 s2)
    MB_NONE,    // 84: lost -- was as 51 (40 -> 240 -> 40, 5x5 s1)
    // column-task depthwise phase for the whole-image late blocks (kernels_mbconv.hip, COLTH): 85..92.  Measured (us per 1 000
    // segments, same box): 344 -> 309 (80 -> 480 -> 112), 493 -> 453 (112 -> 672 -> 112), 337 -> 286 (192 -> 1152 -> 192),
    // 335 -> 298 (192 -> 1152 -> 320).  Tried and dropped: the 3x3 6x32 block with 32-channel chunks (279 against 239 for
    // entry 55's 16-channel chunks) and the Perch-sized 8x32 blocks (8 rows x 5 columns of E in registers: 417 / 604 against
    // 384 / 557).
    //          KS ST KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM
    MB_NONE2,    // 85/86: lost -- was as 34/35 (80 -> 480 -> 112, 6x32)
    MB_NONE2,    // 87/88: lost -- was as 36/37 (112 -> 672 -> 112, 6x32)
    MB_NONE2,    // 89/90: lost -- was as 40/41 (192 -> 1152 -> 192, 3x16 x 2)
    MB_NONE2,    // 91/92: lost -- was as 42/43 (192 -> 1152 -> 320, 3x16 x 2)
    // Perch-sized images (16x63, 8x32 -> 4x16): the entries above need tile heights that leave a ragged second tile row there
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_ENTRY_P(5, 1, 16, 2, 4, 1, 4, 1, 2, 3, 4, 1, 8, 1, 2, 0, 3),    // 93: 40 -> 240 -> 40 at 16x63: 8-row tiles, 16-channel chunks
    MB_ENTRY_P(5, 2, 16, 4, 4, 1, 1, 4, 4, 3, 4, 0, 4, 1, 1, 0, 3),    // 94: 112 -> 672 -> 192, 8x32 -> 4x16 in one tile row
    //          KS ST KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM
    // (measured on the Perch-shaped model, us per 1 000 segments: 1 283 -> 862 with 93, 1 058 -> 555 with 94, 500 -> 431 and
    //  441 -> 393 with 95 / 97; config 4 82 -> 91 k segments/s)
    MB_NONE2,    // 95/96: lost -- was as 75/76 (192 -> 1152 -> 192, 4x16), column tasks
    MB_NONE2,    // 97/98: lost -- was as 77/78 (192 -> 1152 -> 320, 4x16), column tasks
    // 8-wave workgroups (WM x WN = 8: two waves per SIMD inside the ONE workgroup a CU holds of these whole-image tiles), column
    // tasks of two channels per lane (512 per chunk); P1 with the chunk's two column tiles on two waves
    MB_ENTRY_HC(5, 1, 3, 3, 2, 4, 2, 3, 4, 5, 3, 6, 1, 2, 0),           // 99/100: as 85/86 (80 -> 480 -> 112, 6x32)
    MB_ENTRY_HC(5, 1, 4, 3, 2, 4, 2, 3, 4, 5, 3, 6, 1, 2, 0),           // 101/102: as 87/88 (112 -> 672 -> 112, 6x32)
    MB_ENTRY_HC(5, 1, 6, 2, 2, 2, 4, 3, 3, 4, 2, 3, 2, 2, 0),           // 103/104: as 89/90 (192 -> 1152 -> 192, 3x16 x 2)
    MB_ENTRY_HC(3, 1, 6, 1, 1, 2, 4, 3, 5, 4, 2, 3, 2, 2, 0),           // 105/106: as 91/92 (192 -> 1152 -> 320, 3x16 x 2); round 4: no column split (one row tile a wave: 40 B of scratch -> none, 242 -> 236 us)
    MB_ENTRY_HC(5, 1, 6, 2, 2, 4, 2, 2, 6, 4, 2, 4, 2, 2, 0),           // 107/108: as 95/96 (192 -> 1152 -> 192, 4x16 x 2), 8 waves
    MB_ENTRY_HC(3, 1, 6, 1, 1, 4, 2, 2, 10, 4, 2, 4, 2, 2, 0),          // 109/110: as 97/98 (192 -> 1152 -> 320, 4x16 x 2), 8 waves; round 4: no column split (160 B of scratch -> none)
    MB_ENTRY_HC(5, 1, 3, 4, 2, 4, 2, 4, 4, 5, 3, 8, 1, 2, 0),           // 111/112: as 71/72 (80 -> 480 -> 112, 8x32), 8 waves, column tasks (401 -> 358 us; the 112 -> 672 -> 112 twin spills 100 registers: 575 -> 970, removed)
    MB_ENTRY_HC(3, 1, 3, 3, 2, 4, 2, 3, 3, 5, 3, 6, 1, 2, 0),           // 113/114: 80 -> 480 -> 80, 3x3 at 6x32 (as 55, 32-channel chunks), 8 waves, column tasks: 234 -> 221 us
    // Perch-SIZED stack (EfficientNet-B3 widths on the 128 x 497 spectrogram: 64x249, 32x125, 16x63, 8x32, 4x16 images), f16 modes.
    // The 24 / 32 / 48-channel stages run on entries 48-52 and 93; the rest needs 3 / 5 / 8 / 12 k steps and 6-24 project tiles:
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_ENTRY_P(3, 1, 16, 1, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 4, 1, 3),     // 115: stem block, 1-channel spectrogram, 40 -> 24 (as 66 with two project tiles)
    MB_ENTRY_P(3, 1, 32, 1, 3, 1, 4, 1, 2, 2, 4, 2, 8, 1, 2, 1, 1),     // 116: the same, plain f16 (as 47)
    //          KS ST KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM
    MB_ENTRY_HC(3, 1, 3, 4, 2, 4, 2, 4, 3, 5, 3, 8, 1, 2, 0),           // 117/118: 96 -> 576 -> 96, 3x3 at 8x32: 8 waves, column tasks
    // (119-130, round 4: 8 waves, NO column split in the expand phase where the resident A fragments of a split spill -- every wave
    //  its own row tiles and both column tiles of the chunk; the entries they replace are 151-162 below, with the measurements)
    MB_ENTRY_HC(5, 1, 3, 2, 1, 4, 2, 4, 5, 5, 3, 8, 1, 2, 0),           // 119/120: 96 -> 576 -> 136, 5x5 at 8x32
    MB_ENTRY_HC(5, 1, 5, 2, 1, 8, 1, 2, 9, 5, 3, 8, 1, 2, 0),           // 121/122: 136 -> 816 -> 136, 5x5 at 8x32 (project phase as 8 x 1 waves: 72 accumulator registers)
    MB_ENTRY_H(5, 2, 5, 4, 1, 1, 4, 4, 4, 4, 1, 4, 1, 1, 0),            // 123/124: 136 -> 816 -> 232, 5x5 stride 2, 8x32 -> 4x16
    MB_ENTRY_HC(5, 1, 8, 1, 1, 4, 2, 2, 8, 4, 2, 4, 2, 2, 0),           // 125/126: 232 -> 1392 -> 232, 5x5 at 4x16 x 2 segments, 8 waves
    MB_ENTRY_HC(3, 1, 8, 1, 1, 4, 2, 2, 12, 4, 2, 4, 2, 2, 0),          // 127/128: 232 -> 1392 -> 384, 3x3 at 4x16 x 2 segments
    MB_ENTRY_HC(3, 1, 12, 1, 2, 2, 4, 2, 6, 4, 2, 4, 1, 2, 0),          // 129/130: 384 -> 2304 -> 384 at 4x16, one segment, 8 waves (A fragments split by column pair: 96 + 48 accumulator registers)

    // blocks WITHOUT an expand convolution (KG = 0: depthwise -> project + residual, the expand-ratio-1 blocks of EfficientNet after
    // the first; B3 has one at 64x249, 24 channels): the block input is copied into the grid chunk by chunk (mbconv_kernel.hpp)
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_ENTRY_P(3, 1, 16, 0, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 3, 0, 3),     // 131: split-f16 project
    MB_ENTRY_P(3, 1, 16, 0, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 3, 0, 1),     // 132: plain f16 project

    // Small-batch twins of 103-106 (the 3x16 blocks, two segments per workgroup): ONE segment per workgroup, the same chunk and
    // project-tile layout, so the block's weights serve both.  The launcher takes them when a launch has at most one workgroup per
    // CU to offer either way (n <= 256 segments: mb_plan_twin, kernels_mbconv.hip): a 128-segment sub-slice of a host-fed slice or
    // a 256-segment batch (birda's default) fills 64 / 128 CUs with the two-segment tiles and the launch lasts one such tile --
    // 100 us however few segments; one-segment tiles put twice the CUs to work on half the tile each.
    //          KS ST KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM
    MB_ENTRY_HC(5, 1, 6, 1, 2, 2, 4, 2, 3, 4, 2, 3, 1, 2, 0),           // 133/134: 192 -> 1152 -> 192, 3x16, one segment
    MB_ENTRY_HC(3, 1, 6, 1, 1, 2, 4, 2, 5, 4, 2, 3, 1, 2, 0),           // 135/136: 192 -> 1152 -> 320, 3x16, one segment (round 5: no column split, as 105 since round 4 -- with it a one-segment workgroup took 145 us, longer than the two-segment tile's 130)

    // Larger tiles for the two early stride-2 / stride-1 3x3 blocks, re-measured with the degree-5 GELU (round 2's 61 / 62 / 69 lost
    // with the dearer activation): less halo and half the per-tile set-up against a workgroup per CU less.  They lose again
    // (us per 1 000 segments): 16 -> 96 -> 24 890-906 -> 1 016-1 023 (137) / 961-985 (69);
    // 24 -> 144 -> 24 644-654 -> 685-701 (138) / 759-768 (139) -- occupancy hides more than the halo costs.
    //          KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_NONE,    // 137: lost -- was as 69 (16 -> 96 -> 24, tile 8x16) at three waves per SIMD
    MB_NONE,    // 138: lost -- was 24 -> 144 -> 24, tile 12x16 (halo 1.31 against 1.41)
    MB_NONE,    // 139: lost -- was 24 -> 144 -> 24, tile 24x16 = the image's height (halo 1.125)


    // Tile-row-walking twins (the kernel's PERSIST = 2 form, gone with them) of the early-block entries 48 / 49 / 65 / 66 / 50: a workgroup walks one
    // tile column of one segment from the top of the image to the bottom and inherits the last KS - ST expanded rows of every tile
    // from the tile above through an LDS halo store instead of expanding them again (VERDICT r3 next #1).  Parity-green
    // (tools/gpu_block_debug.py), measured (profiles/r4_b_strip_ab.txt, us per 1 000 segments,
    // same box) and REJECTED: stem block 724 -> 767-782, 16 -> 96 -> 24 824 -> 1 037-1 056, 24 -> 144 -> 24 610 -> 842-895,
    // 5x5 stride 2 522 -> 1 014-1 104.  The halo store (5.8 / 15.8 / 25.9 / 75.6 KB) costs workgroups per CU (4 -> 4 / 3 / 2 / 1) and
    // these kernels' time follows the workgroups per CU almost proportionally; at EQUAL occupancy (the stem block) the walk still
    // loses 7 %: the expand phase's critical path is the busiest wave's row tiles (9 tiles over 4 waves = 3, as for the 12 of a
    // plain tile), so the rows that are no longer expanded shorten no phase, while the halo copies and the barrier that ends a
    // tile row lengthen each step (DESIGN.md section 3).
    //          KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_NONE,    // 140: lost -- was as 48 (16 -> 96 -> 24, 48x256 -> 24x128)
    MB_NONE,    // 141: lost -- was as 49 (24 -> 144 -> 24, 24x128)
    MB_NONE,    // 142: lost -- was as 65 (stem block, 2-channel spectrogram)
    MB_NONE,    // 143: lost -- was as 66 (stem block, 1-channel spectrogram)
    MB_NONE,    // 144: lost -- was as 50 (24 -> 144 -> 40, 5x5 stride 2, 24x128 -> 12x64)

    // Occupancy twins (round 4, once the strip walk had shown how closely these kernels' time follows the workgroups per CU): the
    // same tiles with one more wave per SIMD allowed where LDS has room for the extra workgroup.
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_NONE,    // 145: lost -- was as 49 (24 -> 144 -> 24) at four waves per SIMD (33 KB of LDS: four fit)
    MB_NONE,    // 146: lost -- was as 50 (5x5 stride 2) at three
    MB_NONE,    // 147: lost -- was as 51 (5x5 at 12x64) at three
    // Two-wave workgroups on half-width tiles (round 4): twice the independent barrier domains per CU at the same waves per SIMD
    // (7 workgroups of 128 threads fit: 20 KB of LDS each), 3 % more halo for the stride-2 block, 11 % for the stride-1 ones.
    // REJECTED, measured (us per 1 000 segments, medians of 3 alternations on one box, parity green): 780 -> 863 (stem), 890 -> 925,
    // 637 -> 707: each block slower by exactly its extra halo work -- at 3.5-4 waves per SIMD these blocks are VALU-issue bound
    // (ACTIVE_INST_VALU x waves ~ 0.9, profiles/r4_z_sq_counters.txt), so more barrier domains buy nothing and every extra
    // expanded pixel costs its share.
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_NONE,    // 148: lost -- was 16 -> 96 -> 24, tile 4x8 (9 x 17 source rows = 10 row tiles)
    MB_NONE,    // 149: lost -- was stem block, tile 8x8 (10 x 10 = 7 row tiles)
    MB_NONE,    // 150: lost -- was 24 -> 144 -> 24, tile 8x8
    // The Perch-sized late-block entries that 119-130 replaced in round 4, and the alternatives measured beside them
    // (us per 1 000 segments on one box, bench.py --config c4, profiles/r4_k_perch_blocks.txt).  Two things were wrong with
    // them: (1) hipcc sank each window column's FMAs of the 5x5 column tasks below the loads of the next two columns (three columns
    // and their taps in flight, +60 registers; fixed for every 8-wave column task by pinning the sums after each column,
    // mbconv_kernel.hpp MB_P2_PIN): 96 -> 576 -> 136 679 -> 408, 232 -> 1392 -> 232 642 -> 366 with the entries unchanged; (2) the
    // column split of the expand phase keeps every A fragment on two waves; without it:
    //   96 -> 576 -> 136   408 -> 354      136 -> 816 -> 136   794 (4 waves, 532 B of scratch) -> 544
    //   232 -> 1392 -> 232 366 -> 332      232 -> 1392 -> 384  556 (4 waves, one segment) -> 391 (two segments) / 483 (one segment, 177)
    //   384 -> 2304 -> 384 1 110 -> 1 052 (two segments, 396 B of scratch: 161) / 890 (one segment, column pair: now 129)
    // config 4: 46.5 k -> 50.8 k (pin alone) -> 54.4 k segments/s.
    //          KS ST KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM
    MB_NONE2,    // 151/152: lost -- was 136 -> 816 -> 136 with the project phase as 4 x 2 waves (561 against 544)
    MB_NONE2,    // 153/154: lost -- was 119 until round 4
    MB_NONE2,    // 155/156: lost -- was 96 -> 576 -> 96 without the column split (290 against 117's 296: noise)
    MB_NONE2,    // 157/158: lost -- was 125 until round 4
    MB_NONE2,    // 159/160: lost -- was 127 until round 4
    MB_NONE2,    // 161/162: lost -- was 384 -> 2304 -> 384, two segments, no column split (1 052)
    MB_NONE2,    // 163/164: lost -- was 121 until round 4 (4 waves, row tasks)
    // the same for the BirdNET-v2.4-shaped late blocks (no-split twins of 99 / 101 / 113 / 103 / 105): within +-1 % of the split
    // entries there (three k steps: the fragments fit either way), not taken; and the 8-wave twins of 129 / 127
    MB_NONE2,    // 165/166: lost -- was as 99 (80 -> 480 -> 112, 6x32)
    MB_NONE2,    // 167/168: lost -- was as 101 (112 -> 672 -> 112, 6x32)
    MB_NONE2,    // 169/170: lost -- was as 113 (80 -> 480 -> 80, 3x3 at 6x32)
    MB_NONE2,    // 171/172: lost -- was as 103 (192 -> 1152 -> 192, 3x16 x 2)
    MB_NONE2,    // 173/174: lost -- was 105 until round 4 (column split)
    MB_NONE2,    // 175/176: lost -- was 129 until round 4 (4 waves)
    MB_NONE2,    // 177/178: lost -- was 232 -> 1392 -> 384 at 4x16, one segment, 8 waves (483)
    MB_NONE2,    // 179/180: lost -- was 109 until round 4 (column split)
    // Perch-sized stack on the f32 MFMA (v_mfma_f32_16x16x4_f32; the path BH_FLAG_AUTO re-runs a row on): round 3 fused 6 of its 26
    // blocks there.  KG counts 16-deep k steps; 816 and 1392 expanded channels are not multiples of 32, so those blocks run 16-channel
    // chunks (256 column tasks on 512 threads).
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_ENTRY_S(3, 1, 16, 1, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 3, 1),        // 181: stem block, 1-channel spectrogram, 40 -> 24 (as 21 with two project tiles)
    MB_ENTRY_P(3, 1, 16, 0, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 3, 0, 0),     // 182: no-expand block (as 131)
    MB_ENTRY(3, 2, 16, 2, 5, 1, 4, 1, 1, 2, 4, 0, 4, 1, 3),             // 183: 24 -> 144 -> 32, 3x3 stride 2 (as 11 with two k steps)
    MB_ENTRY_PC(3, 1, 32, 6, 2, 1, 4, 2, 4, 3, 5, 3, 8, 1, 2, 0, 0),    // 184: 96 -> 576 -> 96, 3x3 at 8x32, 8 waves, column tasks
    MB_ENTRY_PC(5, 1, 32, 6, 2, 1, 4, 2, 4, 5, 5, 3, 8, 1, 2, 0, 0),    // 185: 96 -> 576 -> 136, 5x5
    MB_ENTRY_PC(5, 1, 16, 9, 2, 1, 8, 1, 2, 9, 5, 3, 8, 1, 2, 0, 0),    // 186: 136 -> 816 -> 136, 5x5
    MB_ENTRY(5, 2, 16, 9, 4, 1, 1, 4, 4, 4, 4, 1, 4, 1, 1),             // 187: 136 -> 816 -> 232, 5x5 stride 2, 8x32 -> 4x16
    MB_ENTRY_PC(5, 1, 16, 15, 1, 1, 4, 2, 2, 8, 4, 2, 4, 2, 2, 0, 0),   // 188: 232 -> 1392 -> 232, 5x5 at 4x16 x 2
    MB_ENTRY_PC(3, 1, 16, 15, 1, 1, 4, 2, 2, 12, 4, 2, 4, 2, 2, 0, 0),  // 189: 232 -> 1392 -> 384, 3x3 at 4x16 x 2
    MB_ENTRY_PC(3, 1, 32, 24, 1, 2, 2, 4, 2, 6, 4, 2, 4, 1, 2, 0, 0),   // 190: 384 -> 2304 -> 384, one segment
    MB_ENTRY_PC(5, 1, 32, 12, 1, 1, 4, 2, 2, 6, 4, 2, 4, 2, 2, 0, 0),   // 191: 192 -> 1152 -> 192, 5x5 at 4x16 x 2 (the B0 plan on a 128-mel spectrogram)
    MB_ENTRY_PC(3, 1, 32, 12, 1, 1, 4, 2, 2, 10, 4, 2, 4, 2, 2, 0, 0),  // 192: 192 -> 1152 -> 320, 3x3 at 4x16 x 2
    // NARROW twins of the BirdNET-shaped late blocks for launches of a few segments (a one-minute file is 20): the same chunk and
    // project-tile layout as 99 / 101 / 113 (6x32 images) and 133 / 135 (3x16), so the block's weights serve them too, on tiles 8
    // columns wide -- four / two workgroups per image instead of one, each expanding its columns' halo again (+50 % / +50 % expanded
    // pixels on a chip that is nine tenths idle at that size).  Bit-identical results: a pixel's sums do not depend on its tile.
    //          KS ST KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM
    MB_ENTRY_HC(5, 1, 3, 2, 2, 4, 2, 1, 4, 3, 3, 6, 1, 2, 0),           // 193/194: 80 -> 480 -> 112, 6x32 in four 6x8 tiles
    MB_ENTRY_HC(5, 1, 4, 2, 2, 4, 2, 1, 4, 3, 3, 6, 1, 2, 0),           // 195/196: 112 -> 672 -> 112
    MB_ENTRY_HC(3, 1, 3, 1, 2, 4, 2, 1, 3, 3, 3, 6, 1, 2, 0),           // 197/198: 80 -> 480 -> 80, 3x3
    MB_ENTRY_HC(5, 1, 6, 1, 2, 2, 4, 1, 3, 3, 2, 3, 1, 2, 0),           // 199/200: 192 -> 1152 -> 192, 3x16 in two 3x8 tiles
    MB_ENTRY_HC(3, 1, 6, 1, 2, 2, 4, 1, 5, 3, 2, 3, 1, 2, 0),           // 201/202: 192 -> 1152 -> 320
    // Measured (tools/gpu_quick_bench.py under rocprofv3 at 20 segments, us per launch): 76.6 -> 47.8
    // (112 -> 672 -> 112), 53.0 -> 33.6, 46.0 -> 24.9 (3x3), 69.7 -> 58.4 and 83.6 -> 66.8 (the 3x16 pair: 36 chunks of weights are
    // the chain there, not the pixels); a forward of 20 segments 1.011 -> 0.824 ms, of 64 1.163 -> 0.973; taken while the narrow
    // tiles number at most 256 (round 5: at 512 launches of 96-256 segments lost 2-4 %, profiles/r5_g_narrow_tiles_sweep.txt; at
    // 1 024 a launch of 192 segments loses 10 %).
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_NONE,    // 203: lost -- was 112 -> 672 -> 192, 5x5 stride 2, 6x32 -> 3x16 in two 3x8 tiles (as 58): 87 -> 91 us, not taken
    // 8-wave workgroups on DOUBLE tiles for the three early blocks (round 4, late): a workgroup's fixed cost -- tile decode, output
    // map, grid zero fill, weight DMA, accumulator set-up: ~1 000 instructions a wave, 39 % of the stem block's time with nothing
    // else running (profiles/r4_m_setup_share.txt) -- paid once per 256 (128) output pixels instead of 128 (64), at the SAME four
    // waves per SIMD (two workgroups of 512 threads per CU instead of four of 256) and less halo (1.27 / 1.10 / 1.27 against 1.41 /
    // 1.16 / 1.41 expanded pixels per output pixel).  REJECTED, measured (us per 1 000 segments, medians of 3 alternations,
    // parity green): stem 778 -> 822, 16 -> 96 -> 24 905 -> 970, 24 -> 144 -> 24 651 -> 920.  Eight waves that meet at every barrier
    // of the chunk loop lose more than the halved fixed cost returns: four independent 4-wave workgroups per CU remain the best
    // shape found for these blocks (strip walking, two-wave tiles, larger 4-wave tiles and these all lost to it).
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_NONE,    // 204: lost -- was stem block, tile 16x16
    MB_NONE,    // 205: lost -- was 16 -> 96 -> 24, tile 8x16 (17 x 33 source pixels = 36 row tiles)
    MB_NONE,    // 206: lost -- was 24 -> 144 -> 24, tile 16x16
    // One-segment twins of 125-128 (the Perch-sized plan's 4x16 stages, two segments per workgroup), round 5: as 133-136 for the
    // 3x16 blocks -- and the only twins a squeeze-excite block takes: its pooled sums come out of the one-segment tile in the very
    // order the two-segment tile adds them (kernels_mbconv.hip mb_twin_sums_match: 64 pixels a segment on 64 thread rows), so a
    // segment's logits still do not depend on the launch.  256 segments a launch: pass A of the seven 232 -> 1 392 blocks had 128
    // workgroups for 256 CUs.
    //          KS ST KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM
    MB_ENTRY_HC(5, 1, 8, 1, 1, 4, 2, 1, 8, 4, 2, 4, 1, 2, 0),           // 207/208: 232 -> 1392 -> 232, 5x5 at 4x16, one segment
    MB_ENTRY_HC(3, 1, 8, 1, 1, 4, 2, 1, 12, 4, 2, 4, 1, 2, 0),          // 209/210: 232 -> 1392 -> 384, 3x3 at 4x16, one segment

#endif
#if MB_PART == 1
    // ---- GENERIC entries (round 6, VERDICT r5 missing #1 / next #1) ---------------------------------------------------------
    // Everything above was shaped for one block of this repo's own plans (and, since round 6, serves any block with FEWER k steps
    // than its own -- the surplus zero-padded -- and, for the column-task entries, any image up to COLTH rows high: mb_try_th's
    // relaxed pass).  The rows below are not shaped for a block but for a CLASS of blocks -- by input width (k steps), output width
    // (project tiles) and depthwise kernel / stride -- on tiles with a full halo, so that any inverted-residual stack a published
    // model file might hold runs fused: row tasks, one segment per workgroup, any image size (the planner shrinks the tile height).
    //   E  Cin <= 64,  Cout <= 64    4 waves        M  Cin <= 128, Cout <= 128   8 waves, 16-channel chunks
    //   L  Cin <= 256, Cout <= 256   8 waves        X  Cin <= 384, Cout <= 512   8 waves, 32-channel chunks, 8-wide tiles
    // Measured against the layer-by-layer path they replace: tools/gpu_plan_coverage.py, profiles/r6_plan_coverage.txt.
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_ENTRY_P(3, 1, 16, 2, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 2, 0, 3),     // 211: E 3x3
    MB_ENTRY_P(3, 2, 16, 2, 5, 1, 4, 1, 1, 4, 4, 0, 4, 1, 2, 0, 3),     // 212: E 3x3 stride 2
    MB_ENTRY_P(5, 1, 16, 2, 4, 1, 4, 1, 2, 4, 4, 1, 8, 1, 2, 0, 3),     // 213: E 5x5
    MB_ENTRY_P(5, 2, 16, 2, 7, 1, 4, 1, 1, 4, 4, 0, 4, 1, 2, 0, 3),     // 214: E 5x5 stride 2
    MB_ENTRY_P(3, 1, 16, 4, 2, 1, 4, 2, 2, 4, 4, 0, 8, 1, 2, 0, 3),     // 215: M 3x3
    MB_ENTRY_P(3, 2, 16, 4, 3, 1, 4, 2, 1, 4, 4, 0, 4, 1, 2, 0, 3),     // 216: M 3x3 stride 2
    MB_ENTRY_P(5, 1, 16, 4, 2, 1, 4, 2, 2, 4, 4, 0, 8, 1, 2, 0, 3),     // 217: M 5x5
    MB_ENTRY_P(5, 2, 16, 4, 4, 1, 4, 2, 1, 4, 4, 0, 4, 1, 2, 0, 3),     // 218: M 5x5 stride 2
    MB_ENTRY_P(3, 1, 32, 8, 1, 1, 2, 4, 2, 4, 4, 0, 4, 1, 2, 0, 3),     // 219: L 3x3
    MB_ENTRY_P(3, 2, 32, 8, 2, 1, 2, 4, 2, 8, 4, 0, 3, 1, 2, 0, 3),     // 220: L 3x3 stride 2 (Cout <= 512: a stride-2 block is where a stack widens)
    MB_ENTRY_P(5, 1, 32, 8, 2, 1, 2, 4, 2, 4, 4, 0, 4, 1, 2, 0, 3),     // 221: L 5x5
    MB_ENTRY_P(5, 2, 32, 8, 2, 1, 2, 4, 2, 8, 4, 0, 3, 1, 2, 0, 3),     // 222: L 5x5 stride 2 (a 6x32 -> 3x16 image is one tile: 192 source rows)
    MB_ENTRY_P(3, 1, 32, 12, 1, 1, 2, 4, 2, 8, 3, 0, 8, 1, 2, 0, 3),    // 223: X 3x3
    MB_ENTRY_P(3, 2, 32, 12, 1, 1, 2, 4, 2, 8, 3, 0, 3, 1, 2, 0, 3),    // 224: X 3x3 stride 2
    MB_ENTRY_P(5, 1, 32, 12, 1, 1, 2, 4, 2, 8, 3, 0, 6, 1, 2, 0, 3),    // 225: X 5x5
    MB_ENTRY_P(5, 2, 32, 12, 1, 1, 2, 4, 2, 8, 3, 0, 1, 1, 2, 0, 3),    // 226: X 5x5 stride 2
    // blocks without an expand convolution (KG = 0): up to 64 output channels on 4 waves, up to 256 on 8
    MB_ENTRY_P(3, 1, 16, 0, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 2, 0, 3),     // 227
    MB_ENTRY_P(3, 2, 16, 0, 5, 1, 4, 1, 1, 4, 4, 0, 4, 1, 2, 0, 3),     // 228
    MB_ENTRY_P(5, 1, 16, 0, 4, 1, 4, 1, 2, 4, 4, 1, 8, 1, 2, 0, 3),     // 229
    MB_ENTRY_P(5, 2, 16, 0, 7, 1, 4, 1, 1, 4, 4, 0, 4, 1, 2, 0, 3),     // 230
    MB_ENTRY_P(3, 1, 32, 0, 1, 1, 2, 4, 2, 4, 4, 0, 4, 1, 2, 0, 3),     // 231
    MB_ENTRY_P(3, 2, 32, 0, 2, 1, 2, 4, 2, 4, 4, 0, 3, 1, 2, 0, 3),     // 232
    MB_ENTRY_P(5, 1, 32, 0, 2, 1, 2, 4, 2, 4, 4, 0, 4, 1, 2, 0, 3),     // 233
    MB_ENTRY_P(5, 2, 32, 0, 2, 1, 2, 4, 2, 4, 4, 0, 2, 1, 2, 0, 3),     // 234
    // stem blocks (3x3 stem conv gathered from the planar spectrogram -> depthwise 3x3 -> project): two- and three-branch front-ends
    // with up to 32 output channels, and every branch count with up to 64 (a first block with another depthwise kernel or stride
    // runs its stem conv as a layer of its own and the rest as a no-expand block)
    MB_ENTRY_P(3, 1, 16, 1, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 4, 2, 3),     // 235: 2-channel spectrogram, Cout <= 32 (as 65 with two project tiles)
    MB_ENTRY_P(3, 1, 16, 2, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 3, 3, 3),     // 236: 3-channel spectrogram (9 runs: two steps)
    MB_ENTRY_P(3, 1, 16, 1, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 3, 1, 3),     // 237: 1 channel, Cout <= 64
    MB_ENTRY_P(3, 1, 16, 1, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 3, 2, 3),     // 238: 2 channels
    MB_ENTRY_P(3, 1, 16, 2, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 3, 3, 3),     // 239: 3 channels
    // ... and the same classes on the f32 MFMA (KG counts 16-deep k steps; the path BH_FLAG_AUTO re-runs an overflowing row on)
    MB_ENTRY_P(3, 1, 16, 4, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 2, 0, 0),     // 240: E
    MB_ENTRY_P(3, 2, 16, 4, 5, 1, 4, 1, 1, 4, 4, 0, 4, 1, 2, 0, 0),     // 241
    MB_ENTRY_P(5, 1, 16, 4, 4, 1, 4, 1, 2, 4, 4, 1, 8, 1, 2, 0, 0),     // 242
    MB_ENTRY_P(5, 2, 16, 4, 7, 1, 4, 1, 1, 4, 4, 0, 4, 1, 2, 0, 0),     // 243
    MB_ENTRY_P(3, 1, 16, 8, 2, 1, 4, 2, 2, 4, 4, 0, 8, 1, 2, 0, 0),     // 244: M
    MB_ENTRY_P(3, 2, 16, 8, 3, 1, 4, 2, 1, 4, 4, 0, 4, 1, 2, 0, 0),     // 245
    MB_ENTRY_P(5, 1, 16, 8, 2, 1, 4, 2, 2, 4, 4, 0, 8, 1, 2, 0, 0),     // 246
    MB_ENTRY_P(5, 2, 16, 8, 4, 1, 4, 2, 1, 4, 4, 0, 4, 1, 2, 0, 0),     // 247
    MB_ENTRY_P(3, 1, 32, 16, 1, 1, 2, 4, 2, 4, 4, 0, 4, 1, 2, 0, 0),    // 248: L
    MB_ENTRY_P(3, 2, 32, 16, 2, 1, 2, 4, 2, 8, 4, 0, 3, 1, 2, 0, 0),    // 249
    MB_ENTRY_P(5, 1, 32, 16, 2, 1, 2, 4, 2, 4, 4, 0, 4, 1, 2, 0, 0),    // 250
    MB_ENTRY_P(5, 2, 32, 16, 2, 1, 2, 4, 2, 8, 4, 0, 3, 1, 2, 0, 0),    // 251
    MB_ENTRY_P(3, 1, 32, 24, 1, 1, 2, 4, 2, 8, 3, 0, 8, 1, 2, 0, 0),    // 252: X
    MB_ENTRY_P(3, 2, 32, 24, 1, 1, 2, 4, 2, 8, 3, 0, 3, 1, 2, 0, 0),    // 253
    MB_ENTRY_P(5, 1, 32, 24, 1, 1, 2, 4, 2, 8, 3, 0, 6, 1, 2, 0, 0),    // 254
    MB_ENTRY_P(5, 2, 32, 24, 1, 1, 2, 4, 2, 8, 3, 0, 1, 1, 2, 0, 0),    // 255
    MB_ENTRY_P(3, 1, 16, 0, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 2, 0, 0),     // 256: no expand convolution
    MB_ENTRY_P(3, 2, 16, 0, 5, 1, 4, 1, 1, 4, 4, 0, 4, 1, 2, 0, 0),     // 257
    MB_ENTRY_P(5, 1, 16, 0, 4, 1, 4, 1, 2, 4, 4, 1, 8, 1, 2, 0, 0),     // 258
    MB_ENTRY_P(5, 2, 16, 0, 7, 1, 4, 1, 1, 4, 4, 0, 4, 1, 2, 0, 0),     // 259
    MB_ENTRY_P(3, 1, 32, 0, 1, 1, 2, 4, 2, 4, 4, 0, 4, 1, 2, 0, 0),     // 260
    MB_ENTRY_P(3, 2, 32, 0, 2, 1, 2, 4, 2, 4, 4, 0, 3, 1, 2, 0, 0),     // 261
    MB_ENTRY_P(5, 1, 32, 0, 2, 1, 2, 4, 2, 4, 4, 0, 4, 1, 2, 0, 0),     // 262
    MB_ENTRY_P(5, 2, 32, 0, 2, 1, 2, 4, 2, 4, 4, 0, 2, 1, 2, 0, 0),     // 263
    MB_ENTRY_S(3, 1, 16, 2, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 3, 2),        // 264: stem block, 2-channel spectrogram, Cout <= 32
    MB_ENTRY_S(3, 1, 16, 2, 3, 1, 4, 1, 2, 2, 4, 1, 8, 1, 3, 3),        // 265: 3 channels (K = 27)
    MB_ENTRY_S(3, 1, 16, 1, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 3, 1),        // 266: 1 channel, Cout <= 64
    MB_ENTRY_S(3, 1, 16, 2, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 3, 2),        // 267: 2 channels
    MB_ENTRY_S(3, 1, 16, 2, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 3, 3),        // 268: 3 channels
#endif
#if MB_PART == 2
    // WHOLE-IMAGE column-task entries for the late stages of a stack nobody tiled (3-8 rows, 16-32 columns, 120-384 channels in,
    // up to 512 out): a late block streams 50-110 KB of weights per chunk whatever its tile holds, so the generic 8-column tiles
    // above (two to four workgroups an image, each streaming everything) lost to the layer-by-layer path there (profiles/
    // r6_plan_coverage_first.txt: 288 -> 1728 -> 288 at 3x16 920 against 770 us per 512 segments).  Column-task entries serve any image up
    // to their height (relaxed pass), so a few cover the family:
    //          KS ST KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM
    MB_ENTRY_HC(5, 1, 12, 1, 2, 2, 4, 2, 8, 4, 2, 4, 1, 2, 0),          // 269/270: up to 4 rows x 16, Cin <= 384, Cout <= 512, 5x5 (as 129)
    MB_ENTRY_HC(3, 1, 12, 1, 2, 2, 4, 2, 8, 4, 2, 4, 1, 2, 0),          // 271/272: the same, 3x3 (129 with 8 project tiles a wave)
    MB_ENTRY_HC(5, 1, 8, 2, 1, 4, 2, 2, 8, 4, 2, 8, 1, 2, 0),           // 273/274: up to 8 rows, 16-column tiles, Cin <= 256, Cout <= 256, 5x5
    MB_ENTRY_HC(3, 1, 8, 2, 1, 4, 2, 2, 8, 4, 2, 8, 1, 2, 0),           // 275/276: 3x3
    MB_ENTRY_HC(5, 1, 12, 1, 1, 2, 4, 2, 8, 3, 2, 8, 1, 2, 0),          // 277/278: up to 8 rows, 8-column tiles, Cin <= 384, Cout <= 512, 5x5
    MB_ENTRY_HC(3, 1, 12, 1, 1, 2, 4, 2, 8, 3, 2, 8, 1, 2, 0),          // 279/280: 3x3
    MB_ENTRY_HC(5, 1, 4, 3, 2, 4, 2, 3, 6, 5, 3, 6, 1, 2, 0),           // 281/282: 6x32 whole image, Cin <= 128, Cout <= 192, 5x5 (101 with 12 project tiles)
    MB_ENTRY_HC(5, 1, 6, 2, 1, 4, 2, 3, 6, 5, 3, 6, 1, 2, 0),           // 283/284: 6x32, Cin <= 192, Cout <= 192, 5x5
    MB_ENTRY_HC(3, 1, 6, 2, 1, 4, 2, 3, 6, 5, 3, 6, 1, 2, 0),           // 285/286: 6x32, Cin <= 192, Cout <= 192, 3x3
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_ENTRY_PC(5, 1, 32, 24, 1, 2, 2, 4, 2, 8, 4, 2, 4, 1, 2, 0, 0),   // 287: as 269 on the f32 MFMA
    MB_ENTRY_PC(3, 1, 32, 24, 1, 2, 2, 4, 2, 8, 4, 2, 4, 1, 2, 0, 0),   // 288: as 271
    MB_ENTRY_PC(5, 1, 32, 16, 2, 1, 4, 2, 2, 8, 4, 2, 8, 1, 2, 0, 0),   // 289: as 273
    MB_ENTRY_PC(3, 1, 32, 16, 2, 1, 4, 2, 2, 8, 4, 2, 8, 1, 2, 0, 0),   // 290: as 275
    MB_ENTRY_PC(5, 1, 32, 24, 1, 1, 2, 4, 2, 8, 3, 2, 8, 1, 2, 0, 0),   // 291: as 277
    MB_ENTRY_PC(3, 1, 32, 24, 1, 1, 2, 4, 2, 8, 3, 2, 8, 1, 2, 0, 0),   // 292: as 279
    // E1: class E for blocks of at most 32 input channels -- ONE k step of resident fragments, so the kernels keep the registers of
    // three or four waves a SIMD like the hand-shaped early entries 48-51 (the two-step E entries hold 150-230 registers: two or
    // three waves; on these vector-issue-bound blocks occupancy is what hides the waits): B0 widths x 1.5, 24 -> 144 -> 36 at 48x256,
    // 984 us per 512 segments on entry 212 against 443 for the 16 -> 96 -> 24 block on entry 48 at 1.5x the work
    //         KS ST CE KG RT NCS WM WN MT NT TWL XBL TH S OCC STEM PREC
    MB_ENTRY_P(3, 1, 16, 1, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 3, 0, 3),     // 293: E1 3x3
    MB_ENTRY_P(3, 2, 16, 1, 5, 1, 4, 1, 1, 4, 4, 0, 4, 1, 4, 0, 3),     // 294: E1 3x3 stride 2
    MB_ENTRY_P(5, 1, 16, 1, 4, 1, 4, 1, 2, 4, 4, 1, 8, 1, 3, 0, 3),     // 295: E1 5x5
    MB_ENTRY_P(5, 2, 16, 1, 7, 1, 4, 1, 1, 4, 4, 0, 4, 1, 3, 0, 3),     // 296: E1 5x5 stride 2
    MB_ENTRY_P(3, 1, 16, 2, 3, 1, 4, 1, 2, 4, 4, 1, 8, 1, 3, 0, 0),     // 297-300: the same on the f32 MFMA (two 16-deep steps)
    MB_ENTRY_P(3, 2, 16, 2, 5, 1, 4, 1, 1, 4, 4, 0, 4, 1, 3, 0, 0),
    MB_ENTRY_P(5, 1, 16, 2, 4, 1, 4, 1, 2, 4, 4, 1, 8, 1, 3, 0, 0),
    MB_ENTRY_P(5, 2, 16, 2, 7, 1, 4, 1, 1, 4, 4, 0, 4, 1, 2, 0, 0),
#endif
