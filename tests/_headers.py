"""What the C headers under include/ declare, read from their text: the reference the host tests hold the ctypes binding to
(tests/test_headers_host.py)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def headers():
    return sorted(h for h in os.listdir(INCLUDE) if h.endswith(".h"))


def _code(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def declared(header):
    """the aslr_ functions the header declares"""
    return set(re.findall(r"\b(aslr_[a-z0-9_]+)\s*\(", _code(header)))


def parameter_counts(header):
    """function -> the number of parameters of its declaration: the commas at the top level of the parameter list plus
    one; (void) and () count as 0"""
    src, out = _code(header), {}
    for m in re.finditer(r"\b(aslr_[a-z0-9_]+)\s*\(", src):
        depth, commas, end = 1, 0, m.end()
        while depth:
            c = src[end]
            depth += (c == "(") - (c == ")")
            commas += c == "," and depth == 1
            end += 1
        inside = src[m.end():end - 1].strip()
        out[m.group(1)] = 0 if inside in ("", "void") else commas + 1
    return out
