"""profiles/jacobian_parity.md is written by several GPU test files, one section each (a section: a line that starts
with "# " up to the next such line).  put_section replaces the caller's section, or appends it, and leaves the others
as they are - whatever order the files run in."""

import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(REPO, "profiles", "jacobian_parity.md")


def put_section(lines, path=None, first=False):
    """lines[0] is the section's heading.  first=True: a new section goes to the top instead of the end."""
    heading = lines[0]
    path = PATH if path is None else path
    try:
        text = open(path).read() if os.path.exists(path) else ""
        sections, current = [], []
        for line in text.splitlines():
            if line.startswith("# ") and current:
                sections.append(current)
                current = []
            current.append(line)
        if current:
            sections.append(current)
        sections = [[*s] for s in sections if any(x.strip() for x in s)]
        new = list(lines)
        for i, s in enumerate(sections):
            if s[0] == heading:
                sections[i] = new
                break
        else:
            sections.insert(0, new) if first else sections.append(new)
        body = "\n\n".join("\n".join(s).rstrip("\n") for s in sections)
        with open(path, "w") as fh:
            fh.write(body + "\n")
    except OSError:                                    # (a read-only checkout: the printed figures remain)
        pass
