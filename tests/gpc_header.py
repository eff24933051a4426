"""include/gpc.h as the table tests read it (test_poison_cpu.py, test_stream_order_cpu.py): the declared entries and, of those, the ones
that enqueue work on the device."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# object calls that launch without carrying _dev in their name
OBJECT_CALLS = {"gpc_sparse_remap", "gpc_registration_step", "gpc_registration_run"}


def header():
    return open(os.path.join(ROOT, "include", "gpc.h")).read()


def declared():
    """as test_capi_cpu.py::test_library_exports_every_declared_symbol reads the header"""
    hdr = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    names = set(re.findall(r"\b(gpc_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) > 80, "no declarations parsed"
    return names


def launching(names):
    dev = {s for s in names if s.endswith("_dev")}
    assert OBJECT_CALLS <= names and len(dev) > 30
    return dev | OBJECT_CALLS


def comment_of(entry):
    """(text, first line, last line) of the last comment that begins a line and ends ahead of the entry's declaration (the comments
    inside a struct follow a member on its line)"""
    hdr = header()
    at = re.search(r"\b%s\s*\(" % re.escape(entry), re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), hdr, flags=re.S)).start()
    last = [m for m in re.finditer(r"^/\*.*?\*/", hdr[:at], flags=re.S | re.M)][-1]
    return last.group(0), hdr.count("\n", 0, last.start()) + 1, hdr.count("\n", 0, last.end()) + 1
