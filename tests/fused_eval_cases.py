"""The convolution cases of the fused inference forward, each with the kernel family it is pinned to: shared by the device
test (bit-identity per family, tests/test_fused_eval_gpu.py) and the host test of the route selection
(tests/test_conv_select_host.py).  The expectations were recorded on an MI355X."""


def R(plain, bits=None, aff2=None, aff2_bits=None):
    """Expected kernel family by operand set: without / with ReLU-bit stores, and with a normalised residual."""
    bits = bits or plain
    return {(False, False): plain, (False, True): bits, (True, False): aff2 or plain, (True, True): aff2_bits or aff2 or bits}


# (id, n, hw, cin, cout, k, stride, chunks, fragments, switches, expected family)
#   cin / cout are the tensors' widths; chunks > 1: grouped, dense inside 64-channel chunks (ResNeXt 32x4d as the engine runs it)
CASES = [
    # 1x1 stride 1, narrow -> wide: the tile kernel, and the register-weight kernel where ReLU bits are stored (its minimum grid)
    ("1x1_64_256_56", 16, 56, 64, 256, 1, 1, 1, None, {}, R("tile_2stage", "regw1x1")),
    ("1x1_128_512_28", 8, 28, 128, 512, 1, 1, 1, None, {}, R("tile_2stage", "regw1x1")),
    ("1x1_256_1024_14", 16, 14, 256, 1024, 1, 1, 1, None, {}, R("tile_2stage", "regw1x1")),
    ("1x1_512_2048_7", 16, 7, 512, 2048, 1, 1, 1, None, {}, R("tile_2stage")),
    ("1x1_64_256_56_no_regw", 16, 56, 64, 256, 1, 1, 1, None, {"IIF_CONV_NO_REGW_FWDBN": "1"}, R("tile_2stage")),
    # ... the streaming kernel (takes the affine when forced; a normalised residual it leaves to the tile kernel)
    ("1x1_64_256_14_stream", 2, 14, 64, 256, 1, 1, 1, None, {"IIF_CONV_STREAM1X1_FORCE": "1", "IIF_CONV_NO_REGW_FWDBN": "1"},
     R("stream1x1", aff2="tile_2stage")),
    ("1x1_256_64_56_stream", 4, 56, 256, 64, 1, 1, 1, None, {"IIF_CONV_STREAM1X1_FORCE": "1"}, R("stream1x1", aff2="tile_2stage")),
    # wide -> narrow
    ("1x1_256_64_56", 16, 56, 256, 64, 1, 1, 1, None, {}, R("tile_2stage")),
    ("1x1_512_128_28", 8, 28, 512, 128, 1, 1, 1, None, {}, R("tile_2stage")),
    ("1x1_1024_256_14", 8, 14, 1024, 256, 1, 1, 1, None, {}, R("tile_2stage")),
    ("1x1_2048_512_7", 16, 7, 2048, 512, 1, 1, 1, None, {}, R("tile_2stage")),
    ("1x1_1024_256_14_bs256", 256, 14, 1024, 256, 1, 1, 1, None, {}, R("tile256")),
    # 1x1 stride 2 (the convolutional shortcut's own geometry)
    ("1x1s2_256_512_56", 8, 56, 256, 512, 1, 2, 1, None, {}, R("tile_2stage")),
    # 3x3 stride 1, 64 channels at 56 px: register-weight kernel; fragment kernel with that one off; tile kernel without fragments
    ("3x3_64_56_regw", 16, 56, 64, 64, 3, 1, 1, "frag", {}, R("regw3x3")),
    ("3x3_64_56_frag", 16, 56, 64, 64, 3, 1, 1, "frag", {"IIF_CONV_NO_REGW": "1"}, R("frag")),
    ("3x3_64_56_tile", 4, 56, 64, 64, 3, 1, 1, None, {"IIF_CONV_NO_REGW": "1"}, R("tile_2stage")),
    # 128 / 256 / 512 channels: halo (128-row at 28 px, 256-row below), 256-row tile, three-stage tile
    ("3x3_128_28_halo", 64, 28, 128, 128, 3, 1, 1, None, {}, R("halo")),
    ("3x3_256_14_halo", 128, 14, 256, 256, 3, 1, 1, None, {}, R("halo")),
    ("3x3_512_7_halo", 256, 7, 512, 512, 3, 1, 1, None, {}, R("halo")),
    ("3x3_256_14_tile256", 256, 14, 256, 256, 3, 1, 1, None, {"IIF_CONV_NO_HALO": "1"}, R("tile256")),
    ("3x3_128_28_tile", 8, 28, 128, 128, 3, 1, 1, None, {}, R("tile_2stage")),
    ("3x3_512_7_tile", 4, 7, 512, 512, 3, 1, 1, None, {}, R("tile")),
    # 3x3 stride 2
    ("3x3s2_128_56", 8, 56, 128, 128, 3, 2, 1, None, {}, R("tile_2stage")),
    ("3x3s2_512_14", 8, 14, 512, 512, 3, 2, 1, None, {}, R("tile")),
    # ResNeXt 32x4d, all four stages: the 16-channel fragment format, the 32-channel one, the tile kernel's grouped path
    ("g3x3_128_56_g16", 8, 56, 128, 128, 3, 1, 2, "g16", {}, R("frag_g16")),
    ("g3x3_256_28_g16", 16, 28, 256, 256, 3, 1, 4, "g16", {}, R("frag_g16")),
    ("g3x3_512_14_g16", 32, 14, 512, 512, 3, 1, 8, "g16", {}, R("frag_g16")),
    ("g3x3_1024_7_frag", 64, 7, 1024, 1024, 3, 1, 16, "frag", {}, R("frag")),
    ("g3x3_128_56_frag", 8, 56, 128, 128, 3, 1, 2, "frag", {}, R("frag")),
    ("g3x3_256_28_tile", 2, 28, 256, 256, 3, 1, 4, None, {}, R("tile_2stage")),
    ("g3x3s2_256_56_tile", 4, 56, 256, 256, 3, 2, 4, None, {}, R("tile_2stage")),
    ("g3x3s2_1024_14_tile", 4, 14, 1024, 1024, 3, 2, 16, None, {}, R("tile_2stage")),
    # CIFAR widths: 16 source channels (general addressing), 32, 64 (register-weight kernel at 8 px), the strided layers, the stem GEMM
    ("c3x3_16_32", 128, 32, 16, 16, 3, 1, 1, None, {}, R("tile_general")),
    ("c3x3_32_16", 128, 16, 32, 32, 3, 1, 1, None, {}, R("tile_2stage")),
    ("c3x3_64_8", 128, 8, 64, 64, 3, 1, 1, None, {}, R("regw3x3")),
    ("c3x3s2_16_32", 128, 32, 16, 32, 3, 2, 1, None, {}, R("tile_general")),
    ("c3x3s2_32_64", 128, 16, 32, 64, 3, 2, 1, None, {}, R("tile_2stage")),
    ("cstem_32_16", 128, 32, 32, 16, 1, 1, 1, None, {}, R("tile_2stage")),
    # m not a multiple of the tile heights (363 and 243 rows)
    ("1x1_128_512_11_ragged", 3, 11, 128, 512, 1, 1, 1, None, {}, R("tile_2stage")),
    ("3x3_64_9_ragged", 3, 9, 64, 64, 3, 1, 1, None, {}, R("tile_2stage")),
]
