"""Mint tests/golden/isaacgym_cli_surface.json from the reference's ppo_continuous_action_isaacgym.py: the ``Args`` field names and
defaults and the TensorBoard tags it writes -- settings and names only.  The module imports ``isaacgym`` at its top and cannot be imported,
so the source is read with ``ast``.

    python tools/mint_isaacgym_goldens.py <path to the reference checkout>
"""
import ast
import json
import os
import sys


def surface(path):
    tree = ast.parse(open(path).read())
    args = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args")
    fields = {}
    for st in args.body:
        if isinstance(st, ast.AnnAssign):
            try:
                fields[st.target.id] = ast.literal_eval(st.value)
            except ValueError:                       # exp_name: derived from the file's name
                fields[st.target.id] = os.path.basename(path)[: -len(".py")]
    tags = [n.args[0].value for n in ast.walk(tree)
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "add_scalar" and isinstance(n.args[0], ast.Constant)]
    episode = [t for t in tags if t.split("/")[1] in ("episodic_return", "episodic_length", "consecutive_successes")]
    return {"fields": fields, "iteration_tags": [t for t in tags if t not in episode], "episode_tags": episode}


if __name__ == "__main__":
    src = os.path.join(sys.argv[1], "cleanrl", "ppo_continuous_action_isaacgym", "ppo_continuous_action_isaacgym.py")
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "isaacgym_cli_surface.json")
    with open(out, "w") as f:
        json.dump(surface(src), f, indent=1)
        f.write("\n")
    print(out)
