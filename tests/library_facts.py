"""Two facts about the built library that the ABI and budget tests read: the public header without its comments, and the resources of
every kernel in the code object.  A helper, not a test."""
import os
import re
import sys

from zoic_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    """include/zoic_amd.h with its comments stripped"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zoic_amd.h")).read(), flags=re.S)


def kernel_resources():
    """tools/code_object_regs.kernel_resources of the built library: kernel name -> registers, spills, scratch, LDS"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import code_object_regs
    finally:
        sys.path.pop(0)
    return code_object_regs.kernel_resources(_capi.LIB_PATH)
