// Stand-alone driver of dbg_assembly_amd/host/kmer_spectrum.h (tests/test_kmer_spectrum_cpu.py builds and runs it, once
// plain and once with -fsanitize=address,undefined).
//   kmer_spectrum_test write <hist.txt>   hist.txt: "k max_freq total_individuals n_rows", then n_rows lines "freq species";
//                                         the spectrum goes to stdout
//   kmer_spectrum_test self               the writer's own rules on small histograms; prints what fails, exit 1 if any
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "kmer_spectrum.h"

using namespace std;

static int failures = 0;

static void expect(bool ok, const char *what, const string &text)
{
	if (ok) return;
	failures++;
	cerr << "FAILED: " << what << "\n" << text << endl;
}

static string spectrum(int k, uint32_t max_freq, const vector<uint64_t> &species, uint64_t individuals)
{
	ostringstream s;
	write_kmer_spectrum(s, k, max_freq, species.data(), individuals);
	return s.str();
}

static const char *kColumns =
    "#Kmer_Frequency\tKmer_Species_Number\tKmer_Species_Ratio\tKmer_Species_accumulate_Ratio\tKmer_Individual_Number"
    "\tKmer_Individual_Ratio\tKmer_Individual_accumulate_ratio\n";

static int self_test()
{
	// the remainder rule: 3 k-mers seen once, 1 seen twice, 1 seen "3 or more" times with 10 individuals in all ->
	// the last row holds 10 - 3 - 2 = 5 individuals and both accumulated columns end at 1
	{
		const string got = spectrum(2, 3, {99, 3, 1, 1}, 10);
		const string want = string("#Kmer size: 2\n#Maximum Kmer frequency: 3\n#Kmer indivdual number: 10\n#Kmer species number: 5\n"
		                           "#Theoretic space of Kmer species: 16  occupied ratio: 0.3125\n\n") + kColumns +
		                    "1\t3\t0.6\t0.6\t3\t0.3\t0.3\n2\t1\t0.2\t0.8\t2\t0.2\t0.5\n3\t1\t0.2\t1\t5\t0.5\t1\n";
		expect(got == want, "remainder rule", got);
	}
	// not cut off: the total equals the sum of freq * species, the last row is freq * species
	{
		const string got = spectrum(2, 3, {0, 3, 1, 1}, 8);
		expect(got.find("\n3\t1\t0.2\t1\t3\t0.375\t1\n") != string::npos, "exact total", got);
	}
	// the empty histogram: every ratio is 0, not nan
	{
		const string got = spectrum(3, 2, {0, 0, 0}, 0);
		const string want = string("#Kmer size: 3\n#Maximum Kmer frequency: 2\n#Kmer indivdual number: 0\n#Kmer species number: 0\n"
		                           "#Theoretic space of Kmer species: 64  occupied ratio: 0\n\n") + kColumns +
		                    "1\t0\t0\t0\t0\t0\t0\n2\t0\t0\t0\t0\t0\t0\n";
		expect(got == want, "empty histogram", got);
	}
	// k = 1: a space of 4 k-mers, all occupied, max_freq = 255 with everything in the last row
	{
		vector<uint64_t> sp(256, 0);
		sp[255] = 4;
		const string got = spectrum(1, 255, sp, 4000);
		expect(got.find("#Theoretic space of Kmer species: 4  occupied ratio: 1\n") != string::npos, "k = 1 header", got);
		expect(got.find("\n254\t0\t0\t0\t0\t0\t0\n255\t4\t1\t1\t4000\t1\t1\n") != string::npos, "k = 1 last row", got);
		size_t lines = 0;
		for (char ch : got) lines += ch == '\n';
		expect(lines == 7 + 255, "k = 1 line count", got);
	}
	return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
	if (argc == 2 && !strcmp(argv[1], "self")) return self_test();
	if (argc != 3 || strcmp(argv[1], "write")) {
		cerr << "usage: kmer_spectrum_test write <hist.txt> | self" << endl;
		return 2;
	}
	ifstream in(argv[2]);
	int k = 0;
	uint32_t max_freq = 0;
	uint64_t individuals = 0, n_rows = 0;
	if (!(in >> k >> max_freq >> individuals >> n_rows)) return 2;
	vector<uint64_t> species((size_t)max_freq + 1, 0);
	for (uint64_t i = 0; i < n_rows; i++) {
		uint64_t f = 0, s = 0;
		if (!(in >> f >> s) || f < 1 || f > max_freq) return 2;
		species[f] = s;
	}
	write_kmer_spectrum(cout, k, max_freq, species.data(), individuals);
	cout.flush();
	return cout ? 0 : 1;
}
