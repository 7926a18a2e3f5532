// simulate_lowfreq_kmer -- correct_error/simulate_lowfreq_kmer.cpp on the GPU: how hard is a genome to correct at this k?
//
// Every k-mer of the genome is marked on both strands in a 4^k-bit table; then every -s bases one base is mutated
// ((code + 1) mod 4) and the k windows over it are looked up: a window the genome does not hold is "low-frequency".
// Printed: genome size, k-mer total and species numbers, the share of low-frequency windows and the share of
// mutations with 100 % / >= 80 % / >= 50 % / >= 20 % / >= 1 such windows -- same command line, usage text and stdout
// as the reference program; the stderr lines carry clock times and differ.
//
// Here the table is what the KFREQ and CORRECT code already build: the sequences are counted by a KFREQ handle (cut
// into pieces that overlap by k - 1 bases, so that every window is counted once whatever the sequence length),
// dbgk_corr_from_kfreq(cutoff 0) marks bit(v) = count[canonical(v)] > 0, and dbgk_corr_mutation_scan looks the
// mutated windows up on the device.
//
// Notes on what differs from the reference:
//   * k is 1..18 (the KFREQ limit); a larger k is refused with a message.
//   * "Kmer species number" is the reference's loop over idx < 4^k - 1: the all-T k-mer is never counted.  The table
//     counts its canonical k-mers while it is built (dbgk_corr_table_stats); every one of them stands for two set
//     bits but those that are their own reverse complement (even k only), which are found on the host.
//   * A record shorter than 2k - 1 bases has no mutation site and one shorter than k has no window; the reference
//     underflows an unsigned length there and aborts.
//   * Bytes outside ACGTNacgtn are read as A (the reference indexes its alphabet table out of bounds).
//   * The reader's rules are the reference's: text before the first '>' is ignored; a record is a header line, then
//     everything up to the next '>' with newlines and spaces removed.
#include <unistd.h>
#include <ctime>
#include <unordered_set>

#include "cli_common.h"

struct Options {
	int k = 17;
	int skip = 100;
	string genome;
};

// the reference's usage text, the defaults as they stand when it is asked for
static void print_usage(const Options &o)
{
	cout << "\nsimulate_lowfreq_kmer <genome_seq*.fa | *.fa.gz>\n"
	        "   -k <int>   set kmer size, default="
	     << o.k << endl
	     << "   -s <int>   set skip distance of muation on reference, default=" << o.skip << endl
	     << "   -h         get the help information\n"
	     << endl
	     << "\n\nInstructions: We simulate each mutation (as sequencing error) along the reference genome with distance 100 bp, one mutation will affect a set of Kmers crossed that site, the number of these Kmers is equal to the Kmer size. We defined low-frequency as a Kmer do not exist in the reference genome, then we calculate the ratio of low-frequency Kmers in each set, and make distribution statistics, to illustrate the difficulty of error correction for each type of genomes.\n"
	     << endl;
}

// false: the usage text was asked for, or there is no genome file
static bool parse_options(int argc, char **argv, Options &o)
{
	for (int opt; (opt = getopt(argc, argv, "k:s:h")) != -1;) {
		if (opt == 'k') o.k = atoi(optarg);
		else if (opt == 's') o.skip = atoi(optarg);
		else return false;
	}
	if (optind >= argc) return false;
	o.genome = argv[optind];
	return true;
}

// the whole file, plain or gzip'ed
static bool slurp(const string &path, string &text)
{
	gzFile f = gzopen(path.c_str(), "rb");
	if (!f) return false;
	gzbuffer(f, 1 << 20);
	vector<char> buf(1 << 22);
	for (int n; (n = gzread(f, buf.data(), (unsigned)buf.size())) > 0;) text.append(buf.data(), (size_t)n);
	gzclose(f);
	return true;
}

// the records' sequences back to back
static void read_genome(const string &text, string &bases, vector<uint64_t> &offsets)
{
	offsets.assign(1, 0);
	size_t at = text.find('>');
	while (at != string::npos && at + 1 < text.size()) {
		const size_t eol = text.find('\n', at + 1); // the header line
		if (eol == string::npos) break;
		const size_t next = text.find('>', eol + 1);
		const size_t end = next == string::npos ? text.size() : next;
		for (size_t i = eol + 1; i < end; i++)
			if (text[i] != '\n' && text[i] != ' ') bases.push_back(text[i]);
		offsets.push_back(bases.size());
		at = next;
	}
}

static unsigned base_code(char ch)
{
	switch (ch & 0xDF) {
		case 'C': return 1;
		case 'G': return 2;
		case 'T': return 3;
		default: return 0; // A, N and every other byte
	}
}

// distinct k-mers of the sequences that equal their own reverse complement (even k; there is none for odd k)
static uint64_t count_palindromes(const string &bases, const vector<uint64_t> &offsets, int k)
{
	if (k % 2) return 0;
	const uint64_t mask = (1ull << (2 * k)) - 1;
	unordered_set<uint64_t> seen;
	for (size_t r = 0; r + 1 < offsets.size(); r++) {
		uint64_t fw = 0, rc = 0;
		for (uint64_t i = offsets[r]; i < offsets[r + 1]; i++) {
			const uint64_t b = base_code(bases[i]);
			fw = ((fw << 2) | b) & mask;
			rc = (rc >> 2) | ((3 - b) << (2 * (k - 1)));
			if (i - offsets[r] + 1 >= (uint64_t)k && fw == rc) seen.insert(fw);
		}
	}
	return seen.size();
}

// share of the mutation sites whose absent windows make up at least `ratio` of the k windows
static double share_at_least(const vector<uint64_t> &bins, double ratio)
{
	const int k = (int)bins.size() - 1;
	uint64_t sites = 0, hit = 0;
	for (int absent = 0; absent <= k; absent++) {
		sites += bins[absent];
		if ((double)absent / k >= ratio) hit += bins[absent];
	}
	return (double)hit / sites;
}

int main(int argc, char *argv[])
{
	Options opt;
	if (!parse_options(argc, argv, opt)) {
		print_usage(opt);
		return 0;
	}
	if (opt.k < 1 || opt.k > 18) {
		cerr << "simulate_lowfreq_kmer: -k " << opt.k << " is outside 1..18, the k-mer sizes the frequency table of this build holds" << endl;
		return 1;
	}
	if (opt.skip < 1) {
		cerr << "simulate_lowfreq_kmer: -s " << opt.skip << " must be at least 1" << endl;
		return 1;
	}
	const clock_t started = clock();
	auto seconds = [&]() { return double(clock() - started) / CLOCKS_PER_SEC; };
	cerr << "\nInput file is: " << opt.genome << "\n\n" << endl;

	cerr << "Begin to construct the reference kmer table:" << endl;
	string bases;
	vector<uint64_t> offsets;
	{
		string text;
		if (!slurp(opt.genome, text)) cerr << "fail to open input file" << opt.genome << endl;
		read_genome(text, bases, offsets);
	}
	const uint64_t n_seqs = offsets.size() - 1, K = (uint64_t)opt.k;
	uint64_t genome_bases = 0, windows = 0;
	for (uint64_t i = 0; i < n_seqs; i++) {
		const uint64_t len = offsets[i + 1] - offsets[i];
		genome_bases += len;
		if (len >= K) windows += len - K + 1;
	}

	// count every window once: pieces of kPiece bases that overlap by k - 1, pushed in batches
	const uint64_t kPiece = 1ull << 20, kBatch = 64ull << 20, step = kPiece - (K - 1);
	dbgk_config cfg;
	memset(&cfg, 0, sizeof cfg);
	cfg.kmer_size = opt.k;
	cfg.max_read_len = (int32_t)kPiece;
	cfg.engine = DBGK_ENGINE_KFREQ;
	cfg.device_id = getenv("DBGK_DEVICE") ? atoi(getenv("DBGK_DEVICE")) : 0;
	cfg.max_batch_bases = kBatch + kPiece;
	dbgk_handle *h = nullptr;
	int rc = dbgk_create(&cfg, &h);
	if (rc) die("dbgk_create", rc);
	{
		string piece_bases;
		vector<uint64_t> piece_off(1, 0);
		auto flush = [&]() {
			if (piece_off.size() > 1) {
				rc = dbgk_push_reads(h, piece_bases.data(), piece_off.data(), piece_off.size() - 1);
				if (rc) die("dbgk_push_reads", rc);
			}
			piece_bases.clear();
			piece_off.assign(1, 0);
		};
		for (uint64_t i = 0; i < n_seqs; i++) {
			const uint64_t len = offsets[i + 1] - offsets[i];
			for (uint64_t at = 0; at + K <= len; at += step) {
				piece_bases.append(bases, offsets[i] + at, min<uint64_t>(kPiece, len - at));
				piece_off.push_back(piece_bases.size());
				if (piece_bases.size() >= kBatch) flush();
			}
		}
		flush();
	}
	dbgk_stats st;
	rc = dbgk_finalize(h, &st);
	if (rc) die("dbgk_finalize", rc);
	if (st.stored_kmers != windows) {
		cerr << "k-mer table: " << st.stored_kmers << " windows counted, " << windows << " expected" << endl;
		return 1;
	}
	dbgk_corr_params cp = {opt.k, 17, 2, 17, 5000000, 75}; // only k matters to the table and the scan
	dbgk_corr *corr = nullptr;
	rc = dbgk_corr_create(&cp, cfg.device_id, &corr);
	if (rc) die("dbgk_corr_create", rc);
	rc = dbgk_corr_from_kfreq(corr, h, 0);
	if (rc) die("dbgk_corr_from_kfreq", rc);
	dbgk_destroy(h);

	// set bits of the table below its last one: two per canonical k-mer, one where it is its own reverse complement
	uint64_t space = 0, canonical = 0;
	rc = dbgk_corr_table_stats(corr, &space, &canonical);
	if (rc) die("dbgk_corr_table_stats", rc);
	uint8_t last_byte = 0;
	rc = dbgk_corr_export_bits(corr, (space - 1) / 8, 1, &last_byte);
	if (rc) die("dbgk_corr_export_bits", rc);
	const uint64_t all_T = (last_byte >> (7 - (space - 1) % 8)) & 1;
	const uint64_t species = 2 * canonical - count_palindromes(bases, offsets, opt.k) - all_T;
	cout << "The Genome size is:  " << genome_bases << endl;
	cout << "Kmer total number:   " << windows << endl;
	cout << "Kmer species number: " << species << endl << endl;
	cerr << "\nFinished time: " << seconds() << endl;

	cerr << "\nBegin to analyze the mutated Kmers:" << endl;
	vector<uint64_t> bins(opt.k + 1, 0); // bins[j]: sites with j of their k windows absent
	rc = dbgk_corr_mutation_scan(corr, bases.data(), offsets.data(), n_seqs, (uint32_t)opt.skip, bins.data());
	if (rc) die("dbgk_corr_mutation_scan", rc);
	dbgk_corr_destroy(corr);

	uint64_t sites = 0, absent_windows = 0;
	for (int j = 0; j <= opt.k; j++) {
		sites += bins[j];
		absent_windows += (uint64_t)j * bins[j];
	}
	cout << "\nKmer size: " << opt.k << endl;
	cout << "\nRatio of low-freq kmers in all kmers by muation : " << (double)absent_windows / (sites * K) << endl;
	cout << "\nRatio of mutations with 100% low-freq kmers:  " << (double)bins[opt.k] / sites << endl;
	cout << "\nRatio of mutations with >=80% low-freq kmers: " << share_at_least(bins, 0.8) << endl;
	cout << "\nRatio of mutations with >=50% low-freq kmers: " << share_at_least(bins, 0.5) << endl;
	cout << "\nRatio of mutations with >=20% low-freq kmers: " << share_at_least(bins, 0.2) << endl;
	cout << "\nRatio of mutations with >= 1 low-freq kmers:  " << (double)(sites - bins[0]) / sites << endl;
	cerr << "\nFinished time: " << seconds() << endl;
	return 0;
}
