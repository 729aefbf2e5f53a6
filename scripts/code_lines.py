#!/usr/bin/env python3
"""Code lines of Python files -- no blank lines, comments or docstrings -- and each file's longest functions (a function's
count includes the functions nested in it).

    python scripts/code_lines.py FILE...
"""
import ast
import io
import sys
import tokenize

NOT_CODE = (tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENCODING,
            tokenize.ENDMARKER)


def code_lines(src: str) -> set[int]:
    doc = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body:
            first = node.body[0]
            if isinstance(first, ast.Expr) and isinstance(first.value, ast.Constant) and isinstance(first.value.value, str):
                doc.update(range(first.lineno, first.end_lineno + 1))
    lines = set()
    for tok in tokenize.generate_tokens(io.StringIO(src).readline):
        if tok.type not in NOT_CODE:
            lines.update(range(tok.start[0], tok.end[0] + 1))
    return lines - doc


def main() -> None:
    total = 0
    for path in sys.argv[1:]:
        src = open(path).read()
        code = code_lines(src)
        funcs = sorted(((sum(n.lineno <= ln <= n.end_lineno for ln in code), n.name) for n in ast.walk(ast.parse(src))
                        if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))), reverse=True)
        total += len(code)
        print(f"{path}: {len(code)} code lines; longest functions: " + ", ".join(f"{name} {n}" for n, name in funcs[:4]))
    print(f"total: {total} code lines")


if __name__ == "__main__":
    main()
