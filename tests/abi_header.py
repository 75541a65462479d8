"""Parser of include/pgx.h shared by the binding tests (test_abi_symbols.py: Python, test_csharp_binding.py: C#)."""
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADER = os.path.join(ROOT, "include", "pgx.h")


def _strip_c_comments(s):
    return re.sub(r"/\*.*?\*/", " ", s, flags=re.S)


def _split_args(a):
    a = a.strip()
    if not a or a == "void":
        return []
    return [x.strip() for x in a.split(",")]


def c_prototypes(text):
    """name -> (return type, [parameter types]) for every pgx_* function of the header text."""
    src = _strip_c_comments(text)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z_0-9 \*]*?)\b(pgx_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3)
        params = []
        for p in _split_args(args):
            p = re.sub(r"\s+", " ", p)
            mm = re.match(r"^(.*?)([A-Za-z_][A-Za-z_0-9]*)$", p)   # the last identifier is the parameter's name
            params.append(mm.group(1).strip() if mm and mm.group(1).strip() else p)
        protos[name] = (re.sub(r"\s+", " ", ret), params)
    return protos


def norm_c(t):
    t = t.replace("const", " ")
    t = re.sub(r"\s+", " ", t).strip()
    return t.replace(" *", "*").replace("* ", "*")
