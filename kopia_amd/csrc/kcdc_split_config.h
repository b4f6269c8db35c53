// Build switches of the splitter kernels (kcdc_split_*.h) and of their host code
// (kcdc_kernels.hip).  Every one of those files includes this first, so all of them see the same
// defaults whichever is read first.  The product builds with all three off; the Makefile's
// instrumented and variants targets turn them on.
#pragma once

#ifndef KCDC_TRACE
#define KCDC_TRACE 0  // timing-trace builds only (tools/trace_pipe.py)
#endif
#ifndef KCDC_DEBUG_CHECKS
#define KCDC_DEBUG_CHECKS 0  // queue invariants checked in the kernels (pcheck; tools/debug_pipe.py)
#endif
#ifndef KCDC_HELP_DIAG
#define KCDC_HELP_DIAG 0  // the batch kernels record lane-divergent control values (kQDiag)
#endif
