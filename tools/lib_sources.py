"""Print the SOURCES list of a multitask_hydranet_amd/_lib.py read from stdin, space separated (tools/ab_head.sh, tools/ab_tree.sh: the A/B
libraries are built from the list the package itself builds, of whichever revision).  The file is parsed, not imported."""
import ast
import re
import sys

print(" ".join(ast.literal_eval(re.search(r"^SOURCES = (\[.*?\])", sys.stdin.read(), re.S | re.M).group(1))))
