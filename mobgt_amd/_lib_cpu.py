"""ctypes binding of libmobgt_cpu.so (include/mobgt_cpu.h): the fork-safe host half of the boundary.  Plain C++ --
no HIP, no threads -- so it may be loaded and called inside forked DataLoader workers (and loading it never imports torch)."""
from ._native import Library

LIBRARY = Library("mobgt_cpu.h", "csrc_cpu", "libmobgt_cpu.so", "MOBGT_CPU_", hip=False,
                  missing="the host algorithms (algos.py) run in it.")
lib, build = LIBRARY.lib, LIBRARY.build
SIGNATURES, CONSTANTS, LIB_PATH = LIBRARY.SIGNATURES, LIBRARY.CONSTANTS, LIBRARY.path
EINDEX, ERECURSION, ENOMEM = LIBRARY.constants("EINDEX", "ERECURSION", "ENOMEM")
