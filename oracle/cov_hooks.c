/* oracle/cov_hooks.c -- TEST INFRASTRUCTURE ONLY, part of the coverage build alone (oracle/Makefile `cov`; the name keeps it out of
 * the orc_*.c wildcard of the port / san / fma builds).  Two exported hooks around libgcov's counters, so that one process can
 * attribute branch outcomes to one input: orc_cov_reset(), run the input, orc_cov_dump(), read the counters
 * (tools_dev/oracle_branches.py). */
void __gcov_reset(void);
void __gcov_dump(void);

void orc_cov_reset(void) { __gcov_reset(); }

/* writes the counters collected since the last reset; libgcov dumps once per reset, so the dump at exit writes nothing more */
void orc_cov_dump(void) { __gcov_dump(); }
