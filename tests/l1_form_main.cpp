// Stand-alone host program for tests/test_l1_form_cpu.py: the level-1 form lists and the decision of
// dbg_assembly_amd/csrc/dbgk_l1_form.h on the CPU -- the header alone, without the kernels and without the HIP runtime.
//   l1_form_main rows                   one line per row of every family's list: "row <form>"; then "count <family> <rows>" per
//                                       family.  Exit status 1 if two rows are equal.
//   l1_form_main plan KEY=VALUE ...     the plan of one batch.  Keys are the fields of L1Facts (part seed kfreq wide wrec kmer_size
//                                       max_read_len n1 kf geom_size size n_reads n_bases has_long uniform_len len_max packed l1_linear
//                                       l1_prefix l1_plain wide_l1_plain); what is not given keeps L1Facts' default.  Prints
//                                       "plan umode=U prefix=P launches=N", then per launch "launch <form> L= W= Q= qmagic= n_lanes=
//                                       lq= tile_blocks= first_read= n_reads= tiles=".  Exit status 1 if a launch's form has no row
//                                       (then "miss <form>" is printed), 2 for a key it does not know.
// Built by the test with the HIP compiler as the other host programs of the suite, host side under ASan + UBSan.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dbgk_l1_form.h"

using namespace dbgk;

static std::vector<L1Form> rows_of(L1Family fam)
{
	std::vector<L1Form> v;
	switch (fam) {
#define ROWS_OF(MAKER, LIST) { const L1Form rows[] = {LIST(MAKER)}; v.assign(rows, rows + sizeof rows / sizeof rows[0]); break; }
#define ROW(...) l1_uniform(__VA_ARGS__),
	case L1Family::Uniform: ROWS_OF(ROW, DBGK_L1_UNIFORM_ROWS)
#undef ROW
#define ROW(...) l1_prefix(__VA_ARGS__),
	case L1Family::Prefix: ROWS_OF(ROW, DBGK_L1_PREFIX_ROWS)
#undef ROW
#define ROW(...) l1_flat(__VA_ARGS__),
	case L1Family::Flat: ROWS_OF(ROW, DBGK_L1_FLAT_ROWS)
#undef ROW
#define ROW(...) l1_flat_lin(__VA_ARGS__),
	case L1Family::FlatLin: ROWS_OF(ROW, DBGK_L1_FLAT_LIN_ROWS)
#undef ROW
#define ROW(...) l1_wide_flat(__VA_ARGS__),
	case L1Family::WideFlat: ROWS_OF(ROW, DBGK_L1_WIDE_FLAT_ROWS)
#undef ROW
#define ROW(...) l1_wide_uniform(__VA_ARGS__),
	case L1Family::WideUniform: ROWS_OF(ROW, DBGK_L1_WIDE_UNIFORM_ROWS)
#undef ROW
#undef ROWS_OF
	}
	return v;
}

static const L1Family kFamilies[] = {L1Family::Uniform, L1Family::Prefix, L1Family::FlatLin, L1Family::Flat, L1Family::WideFlat, L1Family::WideUniform};

static bool has_row(const L1Form &f)
{
	for (const L1Form &r : rows_of(f.family))
		if (r == f) return true;
	return false;
}

int main(int argc, char **argv)
{
	char text[192];
	if (argc == 2 && !strcmp(argv[1], "rows")) {
		int equal = 0;
		for (L1Family fam : kFamilies) {
			const std::vector<L1Form> v = rows_of(fam);
			for (size_t i = 0; i < v.size(); i++) {
				l1_form_text(v[i], text, sizeof text);
				printf("row %s\n", text);
				for (size_t j = 0; j < i; j++) equal += v[i] == v[j];
			}
			printf("count %s %zu\n", l1_family_name(fam), v.size());
		}
		return equal ? 1 : 0;
	}
	if (argc >= 2 && !strcmp(argv[1], "plan")) {
		L1Facts f;
		for (int a = 2; a < argc; a++) {
			const char *eq = strchr(argv[a], '=');
			if (!eq) return 2;
			const size_t n = (size_t)(eq - argv[a]);
			const long long v = strtoll(eq + 1, nullptr, 10);
			auto is = [&](const char *key) { return strlen(key) == n && !strncmp(argv[a], key, n); };
			if (is("part")) f.part = v != 0;
			else if (is("seed")) f.seed = v != 0;
			else if (is("kfreq")) f.kfreq = v != 0;
			else if (is("wide")) f.wide = v != 0;
			else if (is("wrec")) f.wrec = v != 0;
			else if (is("kmer_size")) f.kmer_size = (int)v;
			else if (is("max_read_len")) f.max_read_len = (uint64_t)v;
			else if (is("n1")) f.n1 = (uint32_t)v;
			else if (is("kf")) f.kf = (uint32_t)v;
			else if (is("geom_size")) f.geom_size = (uint64_t)v;
			else if (is("size")) f.size = (uint64_t)v;
			else if (is("n_reads")) f.n_reads = (uint64_t)v;
			else if (is("n_bases")) f.n_bases = (uint64_t)v;
			else if (is("has_long")) f.has_long = (int)v;
			else if (is("uniform_len")) f.uniform_len = v;
			else if (is("len_max")) f.len_max = (uint64_t)v;
			else if (is("packed")) f.packed = v != 0;
			else if (is("l1_linear")) f.l1_linear = (int)v;
			else if (is("l1_prefix")) f.l1_prefix = (int)v;
			else if (is("l1_plain")) f.l1_plain = v != 0;
			else if (is("wide_l1_plain")) f.wide_l1_plain = v != 0;
			else {
				fprintf(stderr, "unknown key in %s\n", argv[a]);
				return 2;
			}
		}
		const L1Plan plan = l1_plan(f);
		printf("plan umode=%d prefix=%d launches=%d\n", plan.umode, (int)plan.prefix, plan.n);
		int missing = 0;
		for (int i = 0; i < plan.n; i++) {
			const L1Launch &l = plan.launch[i];
			l1_form_text(l.form, text, sizeof text);
			printf("launch %s L=%u W=%u Q=%u qmagic=%u n_lanes=%" PRIu64 " lq=%u tile_blocks=%u first_read=%" PRIu64 " n_reads=%" PRIu64 " tiles=%" PRIu64 "\n",
			       text, l.geom.L, l.geom.W, l.geom.Q, l.geom.qmagic, l.geom.n_lanes, l.geom.lq, l.geom.tile_blocks, l.first_read, l.n_reads, l.tiles);
			if (!has_row(l.form)) {
				printf("miss %s\n", text);
				missing++;
			}
		}
		return missing ? 1 : 0;
	}
	fprintf(stderr, "usage: %s rows | plan KEY=VALUE ...\n", argv[0]);
	return 2;
}
