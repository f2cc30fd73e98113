"""The plain C++ part of obj2voxel_amd/csrc/o2v_dev_bits.hpp - the bit grid's struct, word <-> coordinates, membership, faces
and tiles - as text for a host compiler: the host tests of the families that read the bit grid (K12, K14, K16, K20) put it in
front of their own family's plain part, tests/test_host_bits.py compiles it alone."""
import os

BITS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "obj2voxel_amd", "csrc", "o2v_dev_bits.hpp")


def plain_part():
    text = open(BITS).read()
    part = text[text.index("// ---- the layout"):text.index("// ---- wavefronts")]
    return "#define O2V_BITS_HOST\n#define O2V_BITS_FN static inline\n" + part
