// contig_stage.h -- the contig stage of debruijn_contig: graph simplification decided on the host in list order over paths traced on
// the GPU (all walks of a pass at once, against the table as the pass finds it; the host walks a path itself where its trace touches a
// slot changed since), contig read-out on the GPU on the same handle.  Test hook simplify_host=1: no tracing.
//
// Follows build_contig_sequence() of the reference (DBG_contig/contig.cpp:54-102) pass by pass, with its stderr protocol and its
// eight <prefix>.contig.* files.  Linked into bin/debruijn_contig only: a program that links the reference's own contig.cpp next to
// libdbgasm_host.so keeps its own build_contig_sequence() and its own definitions of the -D/-T/... globals.
#ifndef DBGK_HOST_CONTIG_STAGE_H_
#define DBGK_HOST_CONTIG_STAGE_H_

// runs on `kset` as build_debruijn_graph() left it (k <= 31); 0, or a DBGK_ERR_* code of the GPU read-out
int run_contig_stage();
// the same stage on `kset_wide` (k = 33..63, 128-bit k-mers; PARITY UNPINNED above k = 32: the reference stops at 31).  The first
// pass comes with the table from the device (dbgk_wide_export_host_table_links) unless DBGK_LINKS=0 keeps it on the host; the stage
// says on stderr that it is the one on 128-bit k-mers
int run_contig_stage_wide();
// test hook contig_wide (k <= 31): copies `kset` into `kset_wide` with a high word of 0, slot for slot, and runs the wide stage on it.
// Every 128-bit rule is then the reference's 64-bit one, so the files must be the reference's: what anchors the wide stage
int run_contig_stage_wide_on_kset();

#endif
