"""The TOML a dorado-format model directory needs (`config.toml`, src/remora/model_util.py:304-309), without a dependency.

Writer: one level of tables; basic strings, integers, floats (repr: they round-trip), lower-case booleans and one-line arrays
of those; a value that is None is left out, as `toml.dump` leaves it out.

Reader: `tomllib` (Python 3.11) or `tomli` when one is importable; otherwise `parse_subset`, which reads what the writer writes
and what dorado's own model directories hold - `[table]` headers, `key = value` with basic and literal strings, integers,
floats, booleans and one-line arrays of them, comments, blank lines - and refuses everything else with the file and the line
number.  It never guesses at a value.
"""
import math
import re

import numpy as np

from . import RemoraError

_BARE_KEY = re.compile(r"[A-Za-z0-9_-]+\Z")
_INT = re.compile(r"[+-]?(0|[1-9](_?[0-9])*)\Z")
_FLOAT = re.compile(r"[+-]?(0|[1-9](_?[0-9])*)(\.[0-9](_?[0-9])*)?([eE][+-]?[0-9](_?[0-9])*)?\Z")
_ESCAPES = {"b": "\b", "t": "\t", "n": "\n", "f": "\f", "r": "\r", '"': '"', "\\": "\\"}
_ESCAPED = {v: "\\" + k for k, v in _ESCAPES.items()}


# ---- writer --------------------------------------------------------------------------------------------------------------------
def _basic_string(s):
    out = []
    for ch in s:
        if ch in _ESCAPED:
            out.append(_ESCAPED[ch])
        elif ord(ch) < 0x20 or ord(ch) == 0x7F:
            out.append(f"\\u{ord(ch):04x}")
        else:
            out.append(ch)
    return '"' + "".join(out) + '"'


def _key(k):
    k = str(k)
    return k if _BARE_KEY.match(k) else _basic_string(k)


def _value(v, where):
    if isinstance(v, np.generic):
        v = v.item()
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, int):
        return str(v)
    if isinstance(v, float):
        if math.isnan(v):
            return "nan"
        if math.isinf(v):
            return "inf" if v > 0 else "-inf"
        return repr(v)
    if isinstance(v, str):
        return _basic_string(v)
    if isinstance(v, (list, tuple, np.ndarray)):
        items = list(v)
        if any(isinstance(x, (list, tuple, dict, np.ndarray)) or x is None for x in items):
            raise RemoraError(f"toml_lite writes arrays of scalars only ({where})")
        return "[" + ", ".join(_value(x, where) for x in items) + "]"
    raise RemoraError(f"toml_lite cannot write {type(v).__name__} ({where})")


def dumps(doc):
    """{table: {key: value}} -> TOML text, tables and keys in insertion order, None values left out."""
    lines = []
    for table, body in doc.items():
        if not isinstance(body, dict):
            raise RemoraError(f"toml_lite writes one level of tables: top-level key {table!r} is not a table")
        lines.append(f"[{_key(table)}]")
        for k, v in body.items():
            if v is None:
                continue
            if isinstance(v, dict):
                raise RemoraError(f"toml_lite writes one level of tables: {table}.{k} is a table")
            lines.append(f"{_key(k)} = {_value(v, f'{table}.{k}')}")
        lines.append("")
    return "\n".join(lines)


def dump(doc, path):
    with open(path, "w", encoding="utf-8") as fh:
        fh.write(dumps(doc))


# ---- reader --------------------------------------------------------------------------------------------------------------------
class _Line:
    """One line of the subset under a cursor; every refusal names the file and the line."""

    def __init__(self, text, name, lineno):
        self.s, self.i, self.name, self.lineno = text, 0, name, lineno

    def fail(self, what):
        raise RemoraError(f"{self.name}, line {self.lineno}: {what}")

    def skip_ws(self):
        while self.i < len(self.s) and self.s[self.i] in " \t":
            self.i += 1

    def at_end(self):
        """Only white space or a comment is left."""
        self.skip_ws()
        return self.i >= len(self.s) or self.s[self.i] == "#"

    def peek(self):
        return self.s[self.i] if self.i < len(self.s) else ""

    def string(self):
        quote = self.s[self.i]
        if self.s.startswith(quote * 3, self.i):
            self.fail("multi-line strings are not read here")
        self.i += 1
        out = []
        while True:
            if self.i >= len(self.s):
                self.fail("string is not closed on its line")
            ch = self.s[self.i]
            self.i += 1
            if ch == quote:
                return "".join(out)
            if quote == '"' and ch == "\\":
                esc = self.peek()
                self.i += 1
                if esc in _ESCAPES:
                    out.append(_ESCAPES[esc])
                elif esc in ("u", "U"):
                    n = 4 if esc == "u" else 8
                    digits = self.s[self.i : self.i + n]
                    if len(digits) != n or not re.match(r"[0-9A-Fa-f]+\Z", digits):
                        self.fail(f"bad \\{esc} escape")
                    code = int(digits, 16)
                    if code > 0x10FFFF or 0xD800 <= code <= 0xDFFF:
                        self.fail(f"\\{esc}{digits} is no Unicode scalar value")
                    out.append(chr(code))
                    self.i += n
                else:
                    self.fail(f"unknown escape \\{esc}")
            elif (ord(ch) < 0x20 and ch != "\t") or ord(ch) == 0x7F:
                self.fail("control character in a string")
            else:
                out.append(ch)

    def key(self):
        self.skip_ws()
        if self.peek() in ('"', "'"):
            return self.string()
        m = re.compile(r"[A-Za-z0-9_-]+").match(self.s, self.i)
        if not m:
            self.fail("expected a key")
        self.i = m.end()
        return m.group()

    def scalar(self):
        ch = self.peek()
        if ch in ('"', "'"):
            return self.string()
        m = re.compile(r"[^\s,\]#]+").match(self.s, self.i)
        if not m:
            self.fail("expected a value")
        tok = m.group()
        self.i = m.end()
        if tok == "true":
            return True
        if tok == "false":
            return False
        if tok.lstrip("+-") in ("inf", "nan") and len(tok) - len(tok.lstrip("+-")) <= 1:
            return float(tok.replace("+", ""))
        if _INT.match(tok):
            return int(tok.replace("_", ""))
        if _FLOAT.match(tok):
            return float(tok.replace("_", ""))
        self.fail(f"value {tok!r} is not a string, integer, float or boolean (dates, other number bases and nested "
                  "structures are not read here)")

    def value(self):
        self.skip_ws()
        ch = self.peek()
        if ch == "{":
            self.fail("inline tables are not read here")
        if ch != "[":
            return self.scalar()
        self.i += 1
        items = []
        while True:
            self.skip_ws()
            if self.peek() == "]":
                self.i += 1
                return items
            if self.peek() in ("[", "{"):
                self.fail("arrays of arrays or tables are not read here")
            if self.i >= len(self.s) or self.peek() == "#":
                self.fail("array is not closed on its line")
            items.append(self.scalar())
            self.skip_ws()
            if self.peek() == ",":
                self.i += 1
            elif self.peek() != "]":
                self.fail("expected , or ] in an array")


def parse_subset(text, name="<string>"):
    """The subset of the module docstring -> {table: {key: value}} (keys ahead of the first header at the top level)."""
    doc = {}
    table = doc
    for lineno, raw in enumerate(text.split("\n"), 1):
        ln = _Line(raw.rstrip("\r"), name, lineno)
        if ln.at_end():
            continue
        if ln.peek() == "[":
            if ln.s.startswith("[[", ln.i):
                ln.fail("arrays of tables are not read here")
            ln.i += 1
            key = ln.key()
            ln.skip_ws()
            if ln.peek() == ".":
                ln.fail("nested tables are not read here")
            if ln.peek() != "]":
                ln.fail("expected ] after the table name")
            ln.i += 1
            if not ln.at_end():
                ln.fail("text after the table header")
            if key in doc:
                ln.fail(f"table [{key}] defined twice")
            table = doc[key] = {}
            continue
        key = ln.key()
        ln.skip_ws()
        if ln.peek() == ".":
            ln.fail("dotted keys are not read here")
        if ln.peek() != "=":
            ln.fail("expected = after the key")
        ln.i += 1
        val = ln.value()
        if not ln.at_end():
            ln.fail("text after the value")
        if key in table:
            ln.fail(f"key {key!r} defined twice")
        table[key] = val
    return doc


def _stdlib():
    for mod in ("tomllib", "tomli"):
        try:
            return __import__(mod)
        except ImportError:
            pass
    return None


def loads(text, name="<string>"):
    lib = _stdlib()
    if lib is None:
        return parse_subset(text, name)
    try:
        return lib.loads(text)
    except lib.TOMLDecodeError as e:
        raise RemoraError(f"{name}: {e}")


def load(path):
    with open(path, encoding="utf-8") as fh:
        return loads(fh.read(), str(path))
