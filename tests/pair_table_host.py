"""The plain C++ part of obj2voxel_amd/csrc/o2v_dev_pair_table.hpp - the pair key, the hash, the probe run and the first size
of the table in global memory that K23 and K24 fill - as text for a host compiler: the host tests of K23 and K24 put it in front
of their own family's plain part, tests/test_host_pair_table.py compiles it alone."""
import os

PAIR_TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "obj2voxel_amd", "csrc", "o2v_dev_pair_table.hpp")


def plain_part():
    text = open(PAIR_TABLE).read()
    part = text[text.index("// ---- the table:"):text.index("// ---- kernels")]
    return "#define O2V_PT_HOST\n#define O2V_PT_FN static inline\n" + part
