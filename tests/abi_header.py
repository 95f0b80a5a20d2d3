"""The declaration parser the boundary tests share (a helper module, no tests): the `RET rdm_name(PARAMS);` declarations of a public header."""
import re


def declarations(text):
    """[(return type, name, [parameter, ...])] in header order, comments and preprocessor lines stripped; `(void)` is no parameters."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = []
    for m in re.finditer(r"([\w\s*]+?)\b(rdm_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        ret = re.sub(r"\s*\*", "*", " ".join(m.group(1).split()))
        params = [" ".join(p.split()) for p in m.group(3).split(",")]
        out.append((ret, m.group(2), [] if params in ([""], ["void"]) else params))
    return out


def param_type(param):
    """The C type of one parameter without its name and qualifiers: "*" for anything with a `*`, else e.g. "int32_t", "rdm_stream_t"."""
    if "*" in param:
        return "*"
    words = [w for w in param.split() if w != "const"]
    return " ".join(words[:-1] if len(words) > 1 else words)


def stream_taking_declarations(text):
    return [name for _, name, params in declarations(text) if any(re.search(r"\brdm_stream_t\b", p) for p in params)]
