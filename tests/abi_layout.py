"""What the ABI tests share: the functions the headers declare, and a struct's layout as the C compiler sees it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "me_engine.h")).read()
    src += open(os.path.join(ROOT, "include", "me_service.h")).read()
    src += open(os.path.join(ROOT, "include", "me_cluster.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(me_[a-z0-9_]+)\s*\(", src)) - {"me_engine", "me_gen", "me_service", "me_cluster"})


def c_layout(tmp_path, header, struct, fields):
    """sizeof and every offsetof of `struct`, as the C compiler sees the header."""
    src = tmp_path / f"{struct}_layout.c"
    lines = "\n".join(f'  printf("{f} %zu\\n", offsetof({struct}, {f}));' for f in fields)
    src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "{header}"\nint main(void) {{\n'
                   f'  printf("sizeof %zu\\n", sizeof({struct}));\n{lines}\n  return 0;\n}}\n')
    exe = tmp_path / f"{struct}_layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
