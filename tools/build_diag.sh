#!/bin/bash
# Diagnostic variants of libfattn.so (never loaded by the product path; bench.py / tools
# select one with FATTN_LIB=<name>): each drops one phase of the split kernel so the
# phases' costs can be read off the un-instrumented kernel's time.  Built by the
# Makefile's `variant` target (its flags are the library's): lib/libfattn_diag_<name>.so.
set -e
cd "$(dirname "$0")/.."
variant() { make -j"${JOBS:-8}" variant VAR="diag_$1" VFLAGS="${*:2}"; }
variant nocompute -DFATTN_DIAG_NOCOMPUTE
variant notail -DFATTN_DIAG_NOTAIL
variant dmaonly -DFATTN_DIAG_NOCOMPUTE -DFATTN_DIAG_NOTAIL
variant nopublish -DFATTN_DIAG_NOPUBLISH
variant noatomic -DFATTN_DIAG_NOATOMIC
variant nomem -DFATTN_DIAG_NOMEM
variant nomem_notail -DFATTN_DIAG_NOMEM -DFATTN_DIAG_NOTAIL
