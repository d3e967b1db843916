"""Host-side check that the library has one configuration: the environment variables it reads are
exactly the hook table of tools/README.md, no variable name is assembled at run time, and no
`#ifndef S3GRL_*` build-time knob is left."""
import re
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "s3grl_amd" / "csrc"
README = REPO / "tools" / "README.md"


def _csrc_files():
    files = sorted(p for p in CSRC.iterdir() if p.is_file())
    assert files
    return files


def _python_files():
    return sorted((REPO / "s3grl_amd").glob("*.py")) + [REPO / "__graft_entry__.py"]


def _hooks_in_code():
    names = set()
    for p in _csrc_files():
        names |= set(re.findall(r'getenv\(\s*"(S3GRL_\w+)"', p.read_text()))
    env_read = re.compile(r'os\.(?:environ\.get\(|environ\[|getenv\()\s*"(S3GRL_\w+)"')
    for p in _python_files():
        names |= set(env_read.findall(p.read_text()))
    return names


def _hooks_in_readme():
    text = README.read_text()
    start = text.index("## Environment hooks of the library")
    end = text.index("\n## ", start + 1)
    rows = [line for line in text[start:end].splitlines() if line.startswith("| `S3GRL_")]
    names = [re.match(r"\| `(S3GRL_\w+)", line).group(1) for line in rows]
    assert len(names) == len(set(names)), "a variable listed twice"
    return set(names)


def test_hook_table_matches_code():
    code, table = _hooks_in_code(), _hooks_in_readme()
    assert code - table == set(), "read by the library but not in tools/README.md"
    assert table - code == set(), "in tools/README.md but not read by the library"


def test_no_built_names():
    for p in _csrc_files():
        text = p.read_text()
        assert not re.search(r'snprintf\([^;]*"S3GRL_', text), p.name
        # every getenv takes a literal name, so the scan above sees all of them
        assert not re.search(r'getenv\(\s*[^"\s]', text), p.name
    for p in _python_files():
        assert not re.search(r"os\.(?:environ\.get\(|environ\[|getenv\()\s*[^\"\s]", p.read_text()), p.name


def test_no_build_time_hooks():
    found = set()
    for p in _csrc_files():
        found |= set(re.findall(r"^\s*#\s*(?:ifndef|ifdef)\s+(S3GRL_\w+)", p.read_text(), re.M))
        found |= set(re.findall(r"defined\s*\(?\s*(S3GRL_\w+)", p.read_text()))
    assert found == set(), found
